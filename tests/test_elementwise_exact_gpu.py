"""Per-element checks of the memory-bound kernels (csrc/kernels/elementwise.hip) at the sizes and
modes the older tests leave out: rmsnorm's VPT = 8 instantiation and partial last waves, silu_mul
(no test before), the embedding's ``prev`` indirection, rope_kv at D = 64 / ``q_out`` / no slots.
Operands are strided views with sentinel guards (tests/gemm_exact.py, test_gemm_exact_gpu.py)."""
import pytest
import torch

import gemm_exact as X
from test_gemm_exact_gpu import BF16, DEV, Guarded, assert_exact
from vgate import ops
from vgate.ops import reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _native():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ops.native()
    yield


def _within(got, want64, rel, what):
    err = (got.detach().cpu().double() - want64).abs()
    bad = err > rel * want64.abs()
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist(), float((err / want64.abs()).max()))


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("H", [8, 136, 520, 16384])
def test_rmsnorm_per_element(H, residual):
    """H = 8 / 136 / 520: H / 8 is no multiple of 64, the last wave is partly idle; 16384: eight vectors
    per thread. |y - y64| <= 2^-7 |y64|: the kernel rounds to bf16 twice (x * inv, then * w), each
    within 2^-9 relative; the bound is twice their sum. The residual update is bit-exact."""
    g = X._gen(H)
    M, eps = 5, 1e-6
    x = torch.randn(M, H, generator=g).to(BF16)
    r = torch.randn(M, H, generator=g).to(BF16)
    w = (torch.rand(H, generator=g) + 0.5).to(BF16)
    xg, yg = Guarded(M, H, init=x), Guarded(M, H, pad=40)
    rg = Guarded(M, H, init=r, pad=56) if residual else None
    ops.native().rmsnorm(xg.view, rg.view if residual else None, w.to(DEV), yg.view, eps)
    torch.cuda.synchronize()
    for name, b in (("x", xg), ("y", yg), ("res", rg)):
        if b is not None:
            b.assert_guards(f"rmsnorm H={H} {name}")
    s = x
    if residual:
        _, s = ref.rmsnorm_ref(x, w, eps, r)
        assert torch.equal(rg.view.cpu(), s)
    s64 = s.double()
    y64 = s64 * torch.rsqrt(s64.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    _within(yg.view, y64, 2.0 ** -7, f"rmsnorm H={H}")


@pytest.mark.parametrize("M,I", [(3, 72), (520, 8192)])
def test_silu_mul_per_element(M, I):
    """M I / 8 = 27 work items (one partial block) and 532480 (> 2048 blocks x 256 threads: the
    grid-stride loop runs twice). One bf16 rounding (2^-9 relative) plus fp32 exp error far below it:
    |out - ref64| <= 2^-8 |ref64|."""
    g = X._gen(M + I)
    y = (2.0 * torch.randn(M, 2 * I, generator=g)).to(BF16)
    yg, og = Guarded(M, 2 * I, init=y), Guarded(M, I, pad=40)
    ops.native().silu_mul(yg.view, og.view)
    torch.cuda.synchronize()
    yg.assert_guards("silu_mul y")
    og.assert_guards("silu_mul out")
    gate, up = y[:, :I].double(), y[:, I:].double()
    _within(og.view, gate / (1.0 + torch.exp(-gate)) * up, 2.0 ** -8, "silu_mul")


@pytest.mark.parametrize("H", [64, 520])
def test_embedding_prev_indirection(H):
    """Negative ids read the previous step's sample (prev[-id - 1]), which may itself lie inside the
    shard, outside it, or on its edges vstart - 1 | vstart and vstart + rows - 1 | vstart + rows."""
    g = X._gen(H)
    rows, vstart = 40, 50
    table = torch.randn(rows, H, generator=g).to(BF16)
    prev = torch.tensor([50, 89, 90, 49, 70, 5, 300], dtype=torch.int32)
    ids = torch.tensor([-1, 55, -2, 49, -3, 50, -4, 89, -5, 90, -6, 3, -7, 200, 70], dtype=torch.int32)
    T = ids.numel()
    out = torch.full(((T + 4) * H,), X.SENT, dtype=BF16, device=DEV)
    ops.native().embedding(ids.to(DEV), table.to(DEV), out, vstart, prev.to(DEV))
    torch.cuda.synchronize()
    resolved = torch.where(ids < 0, prev[(-ids - 1).clamp(min=0).long()], ids)
    want = ref.embedding_ref(resolved, table, vstart)
    assert bool(want.abs().sum(-1).gt(0).any()) and bool(want.abs().sum(-1).eq(0).any())
    assert torch.equal(out[:T * H].cpu().view(T, H), want)
    assert bool((out[T * H:] == X.SENT).all())
    # without prev a negative id is outside every shard
    out2 = torch.full((T * H,), X.SENT, dtype=BF16, device=DEV)
    ops.native().embedding(ids.to(DEV), table.to(DEV), out2, vstart, None)
    assert torch.equal(out2.cpu().view(T, H), ref.embedding_ref(ids, table, vstart))


@pytest.mark.parametrize("slots_on", [True, False])
@pytest.mark.parametrize("q_out", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_kv_exact(D, q_out, slots_on):
    """Standalone rope_kv on integers with the {0, +1, -1} table: the rotation is a signed permutation,
    so q, k and both caches (sentinel where nothing is written) are known bit patterns. In place and
    into a q_out wider than Hq * D (qkv itself then stays untouched); with and without slots."""
    g = X._gen(D)
    Hq, Hkv, T, blocks, bs = 3, 2, 11, 4, 16
    qkv = torch.randint(-100, 101, (T, (Hq + 2 * Hkv) * D), generator=g).to(BF16)
    cs = X.exact_cos_sin(8, D)
    pos = (torch.arange(T) % 8).int()
    slots = torch.randperm(blocks * bs, generator=g)[:T].int()
    slots[2::4] = -1
    rot, kc64, vc64 = X.rope_expect(qkv, pos, slots if slots_on else None, cs, Hq, Hkv, D, blocks, bs)
    a = qkv.to(DEV)
    kc = torch.full((blocks, Hkv, bs, D), X.SENT, dtype=BF16, device=DEV)
    vc = kc.clone()
    qg = Guarded(T, Hq * D) if q_out else None
    ops.native().rope_kv(a, pos.to(DEV), slots.to(DEV) if slots_on else None, cs.to(DEV), kc, vc, Hq, Hkv, D,
                         qg.view if q_out else None)
    torch.cuda.synchronize()
    if q_out:
        qg.assert_guards("rope_kv q_out")
        assert_exact(qg.view, rot[:, : Hq * D], "q_out")
        assert torch.equal(a.cpu(), qkv)
    else:
        want = rot.clone()
        assert_exact(a, want, "qkv in place")
    assert torch.equal(kc.cpu().double(), kc64) and torch.equal(vc.cpu().double(), vc64)
    assert bool((kc64 == X.SENT).any()) and (not slots_on or bool((kc64 != X.SENT).any()))
