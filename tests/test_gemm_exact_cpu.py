"""CPU side of tests/test_gemm_exact_gpu.py: every parametrised problem is built here, its exactness
preconditions hold, and the project's fp32 references reproduce the float64 expectation bit for
bit, so a GPU failure there is the kernel's and not the test's."""
import pytest
import torch

import gemm_exact as X
import test_gemm_exact_gpu as G
from vgate.ops import reference as ref

SPECS = sorted(G.SPECS, key=repr)


def test_every_family_registered_problems():
    kinds = {s[0] for s in SPECS}
    assert kinds == {"dense", "awq", "silu", "awq_silu", "qkv"}
    assert len(SPECS) > 100


@pytest.mark.parametrize("s", SPECS, ids=lambda s: "-".join(map(str, s)))
def test_problem_preconditions_and_references(s):
    p = G.build(s)
    p.check()  # magnitude bounds, the gate set, float32 == float64 products
    e = p.exp
    assert p.x.dtype == torch.bfloat16 and p.w.dtype == torch.bfloat16
    if p.awq is not None:  # the int4 operands dequantise to exactly w, and s * z is exact
        a = p.awq
        assert int(a["qint"].min()) >= 0 and int(a["qint"].max()) <= 15
        s_ = a["scales"].double()
        assert bool(((s_ == 0.25) | (s_ == 0.5) | (s_ == 1.0)).all())
        assert torch.equal(ref.awq_dequant_ref(a["qint"], a["scales"], a["zeros"], a["group"]), p.w)
        sz = (a["scales"].float() * a["zeros"].float())
        assert torch.equal(sz.to(torch.bfloat16).float(), sz)
    if p.kind == "silu":
        I = p.N // 2
        g = e["gate"]
        assert bool(((g == 0) | (g >= X.GATE_MIN)).all()) and float(g.max()) <= X.BOUND
        # silu(g) == g exactly in fp32 on the gate set
        gf = g.float()
        assert torch.equal(torch.nn.functional.silu(gf), gf)
        assert torch.equal(ref.silu_mul_linear_ref(p.x, p.w[:I], p.w[I:]), e["out"])
        return
    if p.kind == "qkv":
        m = p.qkv
        assert int((m["slots"] < 0).sum()) >= (2 if p.M >= 5 else 0)
        live = m["slots"][m["slots"] >= 0]
        assert live.unique().numel() == live.numel() and int(live.max()) < m["blocks"] * m["bs"]
        assert bool(m["cos_sin"].abs().le(1).all()) and torch.equal(m["cos_sin"], m["cos_sin"].round())
        y = ref.linear_ref(p.x, p.w, p.bias)
        kc = torch.full((m["blocks"], m["hkv"], m["bs"], 128), X.SENT, dtype=torch.bfloat16)
        vc = kc.clone()
        ref.rope_kv_ref(y, m["positions"], m["slots"], m["cos_sin"], kc, vc, m["hq"], m["hkv"], 128)
        assert torch.equal(y[:, : m["hq"] * 128].double(), e["q"])
        assert torch.equal(kc.double(), e["k_cache"]) and torch.equal(vc.double(), e["v_cache"])
        assert bool((e["k_cache"] == X.SENT).any())  # skipped tokens / untouched blocks are in the comparison
        return
    # plain: bf16 / f32 epilogues with bias, separate and in-place residual, whatever the rounding point
    assert torch.equal(ref.linear_ref(p.x, p.w, p.bias).double(), e["biased"])
    assert torch.equal(ref.linear_ref(p.x, p.w, p.bias, out_f32=True).double(), e["biased"])
    assert torch.equal(ref.linear_ref(p.x, p.w, p.bias, p.res).double(), e["full"])
    assert torch.equal(ref.linear_ref(p.x, p.w, None, p.res).double(), G.expected(p, "res"))
    late = (e["biased"] + p.res.double()).to(torch.bfloat16)  # rounding after the residual add instead
    assert torch.equal(late.double(), e["full"])


def test_exact_cos_sin_is_a_signed_permutation():
    cs = X.exact_cos_sin()
    c, s = cs[:, :64], cs[:, 64:]
    assert torch.equal(c * c + s * s, torch.ones_like(c))       # one of the four quarter turns
    assert bool((c[0] == 1).all()) and bool((s[1] == 1).all())   # identity, pure quarter turn
    assert len({tuple(r.tolist()) for r in cs}) == cs.shape[0]   # every position its own pattern


def test_perturb_moves_one_column():
    for s in (G.spec_for("bias", 8, 256, 512), G.spec_for("bias", 8, 256, 512, True)):
        p = G.build(s)
        k = X.active_k(p, p.K // 2)
        pp = X.perturb(p, p.N - 1, k)
        d = (pp.x.double() @ pp.w.double().t()) - p.exp["prod"]
        assert bool((d[:, : p.N - 1] == 0).all()) and bool((d[:, p.N - 1] != 0).any())
        assert torch.equal(d, d.round()) and float(d.abs().max()) >= 1
        assert X.rel_err(p.exp["biased"] + d, p.exp["biased"]) < 1e-2  # invisible to the norm-wise statistic


def test_sentinel_is_exact_and_no_integer():
    t = torch.tensor([X.SENT])
    assert float(t.to(torch.bfloat16).double()) == X.SENT and X.SENT != round(X.SENT)
