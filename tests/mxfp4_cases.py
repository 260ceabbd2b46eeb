"""Integer MXFP4 (e2m1 codes, e8m0 block-32 scales, W4A16) GEMM problems in the style of tests/gemm_exact.py
(helpers of tests/test_mxfp4_gpu.py; exercised without a GPU by tests/test_mxfp4_cpu.py).

The weight is value(code) x 2^(e - 127) with the pair (scale, magnitudes) drawn per (row, 32-block) from
  e = 128 (x 2):   0.5 1 1.5 2 3 4 6  -> 1 2 3 4 6 8 12
  e = 127 (x 1):   1 2 3 4 6          -> 1 2 3 4 6
  e = 126 (x 0.5): 2 4 6              -> 1 2 3
so every weight is an integer and a kernel that applies a neighbouring block's scale produces another
number; x in {-4, 0, 4}: every product is an integer, fp32 accumulation is exact in any order, and every
quantity a kernel may round to bf16 stays within gemm_exact.BOUND = 256, so the expectation (float64, CPU)
is one bit pattern for any K split, wave count or tiles per block.

Densities (measured by running every registered builder below on the CPU): the mean square of these
weights is 19 against 9.5 for fp8_cases' code x scale, so with x at 1/8 and fp8's W at 1/32 one of the 73
registered problems fails Problem.check and the others reach max |x W^T| = 224, which leaves no room for
bias +-8 plus residual +-32. W at 1/64 halves the variance back: every problem passes, measured max
|x W^T| = 192 and max |x W^T + bias + residual| = 200; silu up rows are at a quarter of that density
(measured max 192 over gate and up), and Problem.check decides.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import torch

import gemm_exact as X

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)  # magnitude of code & 7
# (scale byte, admissible magnitude codes): value x 2^(e - 127) is a non-zero integer
FORMS = ((128, (1, 2, 3, 4, 5, 6, 7)), (127, (2, 4, 5, 6, 7)), (126, (4, 6, 7)))
X_DENSITY = 0.125
W_DENSITY = 1.0 / 64


def dequant64(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """float64 value(code) * 2^(e - 127): codes uint8 [N, K] (nibble values), scales uint8 [N, K/32]."""
    mag = E2M1[(codes & 7).long()]
    sign = 1.0 - 2.0 * ((codes >> 3) & 1).double()
    return sign * mag * torch.exp2(scales.double() - 127.0).repeat_interleave(32, dim=1)


@dataclass
class Mxfp4Problem(X.Problem):
    mxfp4: dict | None = None  # codes uint8 [N, K] (one nibble value per byte), scales uint8 [N, K/32]; original rows

    def check(self) -> None:
        super().check()
        codes, scales = self.mxfp4["codes"], self.mxfp4["scales"]
        assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and int(codes.max()) <= 15
        assert tuple(scales.shape) == (self.N, self.K // 32)
        assert torch.equal(dequant64(codes, scales), self.w.double()), "codes x scales is not the problem's weight"


def _draw(N: int, K: int, density: float, g: torch.Generator) -> tuple[torch.Tensor, torch.Tensor]:
    """(codes [N, K], scales [N, K/32]): a form per (row, block), a magnitude of that form and a sign per
    element, thinned to `density` (dropped elements are code 0)."""
    KB = K // 32
    form = torch.randint(0, len(FORMS), (N, KB), generator=g)
    scales = torch.tensor([f[0] for f in FORMS], dtype=torch.uint8)[form]
    pick = torch.randint(0, 1 << 20, (N, K), generator=g)
    mags = torch.zeros(N, K, dtype=torch.long)
    fe = form.repeat_interleave(32, dim=1)
    for i, (_, allowed) in enumerate(FORMS):
        a = torch.tensor(allowed)
        mags = torch.where(fe == i, a[pick % len(a)], mags)
    sign = torch.randint(0, 2, (N, K), generator=g)
    keep = torch.rand((N, K), generator=g) < density
    codes = torch.where(keep, mags | (sign << 3), torch.zeros_like(mags)).to(torch.uint8)
    return codes, scales


def _mx(codes: torch.Tensor, scales: torch.Tensor) -> tuple[dict, torch.Tensor]:
    return dict(codes=codes, scales=scales), X.bf16_exact(dequant64(codes, scales))


@functools.lru_cache(maxsize=None)
def mxfp4_problem(M: int, N: int, K: int, bias: bool = True, res: bool = True, seed: int = 0) -> Mxfp4Problem:
    g = X._gen(7000 * seed + M + 3 * N + 7 * K)
    x = X.bf16_exact(4.0 * X.ternary((M, K), X_DENSITY, g))
    mx, w = _mx(*_draw(N, K, W_DENSITY, g))
    b = X.bf16_exact(torch.randint(-8, 9, (N,), generator=g).double()) if bias else None
    r = X.bf16_exact(torch.randint(-32, 33, (M, N), generator=g).double()) if res else None
    return X._finish_plain(Mxfp4Problem("plain", M, N, K, x, w, b, r, mxfp4=mx))


@functools.lru_cache(maxsize=None)
def mxfp4_silu_problem(M: int, I: int, K: int, seed: int = 0) -> Mxfp4Problem:
    """Rows [gate; up]: x in {0, 4}; gate rows e = 128 with 4 codes of magnitude 3 / 4 / 6 per row (weights 6 / 8
    / 12: gate = 0 or 24..192); up rows as mxfp4_problem at a quarter of its density (half of x is non-zero)."""
    g = X._gen(8000 * seed + M + 3 * I + 7 * K)
    x = X.bf16_exact(4.0 * X.ternary((M, K), 0.5, g, nonneg=True))
    if M > 1:
        x[0] = 0
    cg = torch.zeros(I, K, dtype=torch.uint8)
    cols = torch.rand(I, K, generator=g).topk(4, dim=1).indices
    cg.scatter_(1, cols, torch.tensor([5, 6, 7], dtype=torch.uint8)[torch.randint(0, 3, (I, 4), generator=g)])
    sg = torch.full((I, K // 32), 128, dtype=torch.uint8)
    cu, su = _draw(I, K, W_DENSITY / 4, g)
    mx, w = _mx(torch.cat([cg, cu]), torch.cat([sg, su]))
    return X._finish_silu(Mxfp4Problem("silu", M, 2 * I, K, x, w, mxfp4=mx))


@functools.lru_cache(maxsize=None)
def mxfp4_qkv_problem(M: int, hq: int, hkv: int, K: int, seed: int = 0) -> Mxfp4Problem:
    N = (hq + 2 * hkv) * 128
    base = mxfp4_problem(M, N, K, True, False, seed)
    meta = X.qkv_meta(M, blocks=max(8, (M + 15) // 16 + 2), seed=seed)
    meta.update(hq=hq, hkv=hkv)
    return X._finish_qkv(Mxfp4Problem("qkv", M, N, K, base.x, base.w, base.bias, None, qkv=meta, mxfp4=base.mxfp4))


def _again(p: Mxfp4Problem, codes: torch.Tensor, scales: torch.Tensor) -> Mxfp4Problem:
    assert p.kind == "plain"
    mx, w = _mx(codes, scales)
    return X._finish_plain(Mxfp4Problem("plain", p.M, p.N, p.K, p.x, w, p.bias, p.res, mxfp4=mx))


def perturb(p: Mxfp4Problem, n: int, k: int) -> Mxfp4Problem:
    """The same problem with one code replaced by magnitude 2 (or 4 if it was 2), an integer under each of
    the three scales: only output column n may change."""
    codes = p.mxfp4["codes"].clone()
    codes[n, k] = 4 if int(codes[n, k]) & 7 != 4 else 6
    return _again(p, codes, p.mxfp4["scales"])


def perturb_scale(p: Mxfp4Problem, n: int, kb: int) -> Mxfp4Problem:
    """The same problem with the scale of block (row n, k-block kb) moved by one binade (127 <-> 128,
    126 -> 127): with x = +-4 every product stays an integer; only output column n may change."""
    scales = p.mxfp4["scales"].clone()
    scales[n, kb] = 128 if int(scales[n, kb]) == 127 else 127
    return _again(p, p.mxfp4["codes"], scales)


def active_block(p: Mxfp4Problem, n0: int = 0) -> tuple[int, int]:
    """(n, kb): the first output column n >= n0 and its first k-block whose partial product x W[n, block]^T is
    non-zero in some row of x (so a change of that block's scale shows in column n)."""
    part = torch.einsum("mbk,nbk->mnb", p.x.double().reshape(p.M, -1, 32), p.w.double().reshape(p.N, -1, 32))
    nz = (part != 0).any(0).nonzero()
    n, kb = nz[nz[:, 0] >= n0][0].tolist()
    return n, kb


def active_code(p: Mxfp4Problem, n: int, k0: int = 0) -> int:
    """A column k >= k0 with x non-zero in some row (gemm_exact.active_k)."""
    return X.active_k(p, k0)


# ------------------------------------------------------------------ the registered problems
SPECS: set = set()
_BUILDERS = {"plain": mxfp4_problem, "silu": mxfp4_silu_problem, "qkv": mxfp4_qkv_problem}
QKV_HEADS = (2, 1)  # the QKV problem brings its own N = 512


def spec_for(mode: str, M: int, N: int, K: int):
    if mode == "silu":
        s = ("silu", M, N // 2, K)
    elif mode == "qkv":
        s = ("qkv", M) + QKV_HEADS + (K,)
    else:
        s = ("plain", M, N, K)
    SPECS.add(s)
    return s


def build(s) -> Mxfp4Problem:
    return _BUILDERS[s[0]](*s[1:])


DEC_M = [1, 5, 8, 9, 16]
ODD_N = 16 * 37
DEC_MODES = ["bias", "res", "inplace", "f32", "silu", "qkv"]
# (id, N, K, knobs): the launcher's own plan on every shape, then forced K slices 2 / 3 / 8 with 2 / 4 waves
DEC_CASES = [
    ("auto", 256, 512, {}),
    ("auto_k1536", ODD_N, 1536, {}),
    ("auto_k2048", 256, 2048, {}),
    ("w4s2_granules", 256, 512, dict(waves=4, splitk=2)),
    ("w4s3", ODD_N, 1536, dict(waves=4, splitk=3)),
    ("w2s8", 256, 2048, dict(waves=2, splitk=8)),
    # 2 / 4 tiles per block (QKV keeps one); 37 tiles do not divide by 2 or 4: one tile per block
    ("ntb2_w4s3", 256, 1536, dict(waves=4, splitk=3, ntb=2)),
    ("ntb4_w2", 256, 2048, dict(waves=2, splitk=1, ntb=4)),
    ("ntb2_odd", ODD_N, 512, dict(waves=4, splitk=1, ntb=2)),
    ("ntb4_odd", ODD_N, 512, dict(waves=2, splitk=2, ntb=4)),
]
# the launcher's own tiles-per-block rule (gemm_mxfp4.hip mxfp4_ntb_rule): (first tile count, tiles per block),
# and one wide N just above each change, divisible by its count
NTB_RULE = [(0, 1), (1024, 4)]
WIDE_CASES = [(M, mode, 16 * (t + ntb), ntb) for t, ntb in NTB_RULE[1:] for M, mode in ((5, "inplace"), (16, "silu"))]
DEQ_SHAPES = [(256, 512), (ODD_N, 1536)]
DEQ_M = [17, 64, 129]

for _id, _N, _K, _kw in DEC_CASES:
    for _M in DEC_M:
        for _mode in DEC_MODES:
            spec_for(_mode, _M, _N, _K)
for _M, _mode, _N, _ntb in WIDE_CASES:
    spec_for(_mode, _M, _N, 512)
for _N, _K in DEQ_SHAPES:
    for _M in DEQ_M:
        spec_for("bias", _M, _N, _K)


# ------------------------------------------------------------------ every code
EVERY_CODE_SCALES = (2, 3, 64, 100, 120, 126, 127, 128, 129, 134, 150, 190, 220, 250, 251, 252)


def every_code_table() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(codes uint8 [16, 512], scales uint8 [16, 16], x bf16 [16, 512], k_m): x row m is one-hot at
    k_m = 32 m + (5 m + 3) % 32, one column in each of the 16 blocks of K = 512; row n of the single tile
    holds code n at every k_m; block m carries the scale byte EVERY_CODE_SCALES[m] in every row (both ends of
    the admitted range 2..252 and the three binades around 1). out[m][n] is then value(n) x 2^(e_m - 127).
    Rows 0 and 8 (codes +0 and -0) are all-zero blocks, whose scale the Linear rewrites to 127."""
    m = torch.arange(16)
    km = 32 * m + (5 * m + 3) % 32
    codes = torch.zeros(16, 512, dtype=torch.uint8)
    codes[:, km] = torch.arange(16, dtype=torch.uint8)[:, None].expand(16, 16)
    scales = torch.tensor(EVERY_CODE_SCALES, dtype=torch.uint8)[None].expand(16, 16).contiguous()
    x = torch.zeros(16, 512, dtype=torch.bfloat16)
    x[m, km] = 1.0
    return codes, scales, x, km


def every_code_values() -> torch.Tensor:
    """float64 [m][n] = value(n) x 2^(EVERY_CODE_SCALES[m] - 127), -0 for code 8."""
    v = torch.cat([E2M1, -E2M1])  # [n]
    return v[None] * torch.exp2(torch.tensor(EVERY_CODE_SCALES, dtype=torch.float64) - 127.0)[:, None]
