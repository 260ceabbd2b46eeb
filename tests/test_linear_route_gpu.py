"""``ops.linear`` reaches the kernel its route names: one representative per route, on the GPU.

tests/test_linear_route_cpu.py pins the ``C.gemm`` arguments of every route without a GPU; here each
route's ``ops.linear`` call runs under the launch timeline next to a direct ``C.gemm`` call with that
route's knobs. Both must launch the same kernels (the ``tl_take`` names, literal below) and write the
same bits: the operands are the integer problems of tests/gemm_exact.py, whose result is one bit
pattern whatever the K split or summation order. (``awq_dequant`` takes no timeline entry: the dequant
route shows as the bf16 kernels that follow it, and in the compared output.)
"""
from __future__ import annotations

import pytest
import torch

import gemm_exact as X
from vgate import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = 512
MID4 = ops.MID_BASE - 4

# id, AWQ, M, N, Linear attributes, the C.gemm knobs of the route (None: the dequant route), launch names
ROUTES = [
    ("dense_auto", False, 4, 256, {}, {}, ["gemm"]),
    ("dec_path_kx", False, 4, 256, dict(dec_path=4), dict(path=4), ["kx"]),
    # 16 tiles x 4 packed k-steps are fewer units than CUs: the stream-K launcher declines N = 256
    ("dec_sk_declined", False, 4, 256, dict(dec_sk=(8, 1, 4)), dict(path=3, waves=8, splitk=1, ntb=4), ["gemm"]),
    ("dec_sk", False, 4, 1024, dict(dec_sk=(8, 1, 4)), dict(path=3, waves=8, splitk=1, ntb=4), ["gemm_sk_o"]),
    ("mid_plan", False, 48, 256, dict(prefill_plan={48: (MID4, 1)}), dict(path=2, waves=4, splitk=1), ["gemm_mid"]),
    ("prefill_plan", False, 128, 256, dict(prefill_plan={128: (128, 2)}), dict(path=1, ntb=128, splitk=2),
     ["gemm_prefill", "prefill_reduce"]),
    ("awq_decode", True, 4, 256, {}, {}, ["awq_kx"]),
    ("awq_mid", True, 48, 256, {}, dict(path=2), ["awq_mid", "prefill_reduce"]),  # (its own K split at K = 512)
    ("awq_dequant", True, 128, 256, {}, None, ["gemm_prefill", "prefill_reduce"]),
]


def make_lin(p: X.Problem, attrs: dict) -> ops.Linear:
    bias = p.bias.to(DEV)
    if p.awq is not None:
        a = p.awq
        lin = ops.Linear(None, bias=bias, awq=dict(qint=a["qint"], scales=a["scales"].to(DEV),
                                                   zeros=a["zeros"].to(DEV), group=a["group"]))
    else:
        lin = ops.Linear(p.w.to(DEV), bias=bias)
    for k, v in attrs.items():
        setattr(lin, k, v)
    return lin


@pytest.mark.parametrize("awq,M,N,attrs,knobs,names", [r[1:] for r in ROUTES], ids=[r[0] for r in ROUTES])
def test_linear_launches_its_route(awq, M, N, attrs, knobs, names):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    C = ops.native()
    p = X.awq_problem(M, N, K) if awq else X.dense_problem(M, N, K)
    lin = make_lin(p, attrs)
    x = p.x.to(DEV)
    got = {}

    def via_linear():
        got["linear"] = ops.linear(x, lin)

    def direct():
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        kw = dict(bias=lin.bias, ws=ops.workspace(DEV))
        wp = lin.wp
        if knobs is None:  # int4 -> bf16 scratch, then the bf16 kernels on their own rule
            wp = torch.empty(N * K, dtype=torch.bfloat16, device=DEV)
            C.awq_dequant(lin.wp, lin.scales, lin.zeros, N, K, lin.group, wp, None)
        else:
            kw.update(knobs, fault=ops.fault_word(DEV))
            if M <= 16:
                kw["sk_ws"] = ops.sk_workspace(DEV)
            if awq:
                kw.update(awq_scales=lin.scales, awq_zeros=lin.zeros, group=lin.group, awq_szp=lin.szp)
        C.gemm(x, wp, N, K, out, 0, **kw)
        got["direct"] = out

    fault0 = int(ops.fault_word(DEV)[0])
    ran = {k: [e[0] for e in X.launches(fn)] for k, fn in (("linear", via_linear), ("direct", direct))}
    print(f"route launches: {ran}")
    assert ran["linear"] == names and ran["direct"] == names, (ran, names)
    assert torch.equal(got["linear"], got["direct"])
    assert torch.equal(got["linear"].cpu().double(), p.exp["biased"])
    assert int(ops.fault_word(DEV)[0]) == fault0
