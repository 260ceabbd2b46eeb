"""Integer FP8 (e4m3fn, W8A16) GEMM problems in the style of tests/gemm_exact.py (helpers of
tests/test_fp8_gpu.py; exercised without a GPU by tests/test_fp8_cpu.py).

The weight is code x scale with codes drawn from integers that e4m3 holds exactly and power-of-two scales,
x in {-4, 0, 4}: every product is an integer, fp32 accumulation is exact in any order, and every
quantity a kernel may round to bf16 stays within gemm_exact.BOUND = 256, so the expectation (float64, CPU)
is one bit pattern wherever a kernel applies the scale or rounds.

Densities: x at 1/8 and W at 1/16 gave max |x W^T| = 222 at K <= 2048, N <= 592, which leaves no room
for bias +-8 plus residual +-32; W is thinned to 1/32 here (a quarter of the variance of that sum's terms
removed; measured max 192, and 218 with bias and residual), and Problem.check decides.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import torch

import gemm_exact as X

E4M3_INTS = torch.tensor([1.0, 2.0, 3.0, 4.0, 6.0, 8.0], dtype=torch.float64)
X_DENSITY = 0.125
W_DENSITY = 1.0 / 32
SCALE_FORMS = ("channel", "block")


@dataclass
class Fp8Problem(X.Problem):
    fp8: dict | None = None  # codes uint8 [N, K] (e4m3fn), scales fp32 [G, N], G = 1 | K / 128; original row order

    def check(self) -> None:
        super().check()
        codes, scales = self.fp8["codes"], self.fp8["scales"]
        G = scales.shape[0]
        s = scales.double().t().repeat_interleave(self.K // G, dim=1)  # [N, K]
        vals = codes.view(torch.float8_e4m3fn).double()
        assert bool(torch.isfinite(vals).all())
        assert torch.equal(vals * s, self.w.double()), "codes x scales is not the problem's weight"


def codes_of(vals: torch.Tensor) -> torch.Tensor:
    """float64 values -> e4m3fn codes (uint8), asserting nothing is lost."""
    c = vals.to(torch.float8_e4m3fn)
    assert torch.equal(c.double(), vals), "value not representable in e4m3"
    return c.view(torch.uint8)


def _weights(N: int, K: int, density: float, g: torch.Generator) -> torch.Tensor:
    """float64 [N, K]: +-{1, 2, 3, 4, 6, 8} thinned to `density`."""
    mag = E4M3_INTS[torch.randint(0, len(E4M3_INTS), (N, K), generator=g)]
    sign = torch.randint(0, 2, (N, K), generator=g).double() * 2 - 1
    keep = (torch.rand((N, K), generator=g) < density).double()
    return mag * sign * keep


def _scales(N: int, K: int, form: str, g: torch.Generator) -> torch.Tensor:
    """fp32 [G, N] powers of two in {0.25, 0.5, 1}: G = 1 per channel, K / 128 per block."""
    G = 1 if form == "channel" else K // 128
    return (0.25 * 2.0 ** torch.randint(0, 3, (G, N), generator=g).double()).float()


def _fp8_from(vals: torch.Tensor, scales: torch.Tensor) -> tuple[dict, torch.Tensor]:
    N, K = vals.shape
    s = scales.double().t().repeat_interleave(K // scales.shape[0], dim=1)
    return dict(codes=codes_of(vals), scales=scales), X.bf16_exact(vals * s)


@functools.lru_cache(maxsize=None)
def fp8_problem(M: int, N: int, K: int, form: str = "channel", bias: bool = True, res: bool = True,
                seed: int = 0) -> Fp8Problem:
    g = X._gen(5000 * seed + M + 3 * N + 7 * K + (11 if form == "block" else 0))
    x = X.bf16_exact(4.0 * X.ternary((M, K), X_DENSITY, g))
    fp8, w = _fp8_from(_weights(N, K, W_DENSITY, g), _scales(N, K, form, g))
    b = X.bf16_exact(torch.randint(-8, 9, (N,), generator=g).double()) if bias else None
    r = X.bf16_exact(torch.randint(-32, 33, (M, N), generator=g).double()) if res else None
    return X._finish_plain(Fp8Problem("plain", M, N, K, x, w, b, r, fp8=fp8))


@functools.lru_cache(maxsize=None)
def fp8_silu_problem(M: int, I: int, K: int, form: str = "channel", seed: int = 0) -> Fp8Problem:
    """Rows [gate; up]: x in {0, 4}; gate rows scale 1 with 4 codes in {6, 8} per row (gate = 0 or
    24..128); up rows as fp8_problem at a quarter of its density (half of x is non-zero here)."""
    g = X._gen(6000 * seed + M + 3 * I + 7 * K + (11 if form == "block" else 0))
    x = X.bf16_exact(4.0 * X.ternary((M, K), 0.5, g, nonneg=True))
    if M > 1:
        x[0] = 0
    wg = torch.zeros(I, K, dtype=torch.float64)
    cols = torch.rand(I, K, generator=g).topk(4, dim=1).indices
    wg.scatter_(1, cols, 6.0 + 2.0 * torch.randint(0, 2, (I, 4), generator=g).double())
    wu = _weights(I, K, W_DENSITY / 4, g)
    s = _scales(2 * I, K, form, g)
    s[:, :I] = 1.0
    fp8, w = _fp8_from(torch.cat([wg, wu]), s)
    return X._finish_silu(Fp8Problem("silu", M, 2 * I, K, x, w, fp8=fp8))


@functools.lru_cache(maxsize=None)
def fp8_qkv_problem(M: int, hq: int, hkv: int, K: int, form: str = "channel", seed: int = 0) -> Fp8Problem:
    N = (hq + 2 * hkv) * 128
    base = fp8_problem(M, N, K, form, True, False, seed)
    meta = X.qkv_meta(M, blocks=max(8, (M + 15) // 16 + 2), seed=seed)
    meta.update(hq=hq, hkv=hkv)
    return X._finish_qkv(Fp8Problem("qkv", M, N, K, base.x, base.w, base.bias, None, qkv=meta, fp8=base.fp8))


def perturb(p: Fp8Problem, n: int, k: int) -> Fp8Problem:
    """The same problem with one code replaced by another exact integer: only output column n may change."""
    codes = p.fp8["codes"].clone()
    old = float(codes[n, k].view(torch.float8_e4m3fn))
    new = 2.0 if old != 2.0 else 3.0
    codes[n, k] = codes_of(torch.tensor(new, dtype=torch.float64))
    G = p.fp8["scales"].shape[0]
    w = p.w.clone()
    w[n, k] = new * float(p.fp8["scales"][k // (p.K // G), n])
    return Fp8Problem(p.kind, p.M, p.N, p.K, p.x, w, p.bias, p.res, qkv=p.qkv, fp8=dict(p.fp8, codes=codes))


# ------------------------------------------------------------------ the registered problems
SPECS: set = set()
_BUILDERS = {"plain": fp8_problem, "silu": fp8_silu_problem, "qkv": fp8_qkv_problem}
QKV_HEADS = (2, 1)  # the QKV problem brings its own N = 512


def spec_for(mode: str, M: int, N: int, K: int, form: str):
    if mode == "silu":
        s = ("silu", M, N // 2, K, form)
    elif mode == "qkv":
        s = ("qkv", M) + QKV_HEADS + (K, form)
    else:
        s = ("plain", M, N, K, form)
    SPECS.add(s)
    return s


def build(s) -> Fp8Problem:
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
    # 2 / 4 tiles per block (QKV keeps one); 37 tiles do not divide by 2: one tile per block
    ("ntb2_w4s3", 256, 1536, dict(waves=4, splitk=3, ntb=2)),
    ("ntb4_w2", 256, 2048, dict(waves=2, splitk=1, ntb=4)),
    ("ntb2_odd", ODD_N, 512, dict(waves=4, splitk=1, ntb=2)),
]
WIDE_N = 16 * 1026  # from 1024 tiles up the launcher's own plan puts two tiles in a block
WIDE_CASES = [(M, mode, form) for M in (5, 16) for mode, form in (("inplace", "block"), ("silu", "channel"))]
DEQ_SHAPES = [(256, 512), (ODD_N, 1536)]
DEQ_M = [17, 64, 129]

for _id, _N, _K, _kw in DEC_CASES:
    for _M in DEC_M:
        for _mode in DEC_MODES:
            for _form in SCALE_FORMS:
                spec_for(_mode, _M, _N, _K, _form)
for _M, _mode, _form in WIDE_CASES:
    spec_for(_mode, _M, WIDE_N, 512, _form)
for _N, _K in DEQ_SHAPES:
    for _M in DEQ_M:
        for _form in SCALE_FORMS:
            spec_for("bias", _M, _N, _K, _form)


def every_code_table() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(codes uint8 [16, 512], x bf16 [16, 512], k_m): W[n][k_m] is code 16 m + n (the two NaN codes
    replaced by 0), x row m is one-hot at k_m = 33 m, so out[m][n] is the value of code 16 m + n."""
    km = 33 * torch.arange(16)
    codes = torch.zeros(16, 512, dtype=torch.uint8)
    c = (16 * torch.arange(16)[None, :] + torch.arange(16)[:, None]).to(torch.uint8)  # [n][m]
    c[(c & 0x7F) == 0x7F] = 0
    codes[:, km] = c
    x = torch.zeros(16, 512, dtype=torch.bfloat16)
    x[torch.arange(16), km] = 1.0
    return codes, x, km
