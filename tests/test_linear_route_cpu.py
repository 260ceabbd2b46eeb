"""Which kernel ``ops.linear`` asks for, pinned without a GPU.

The real ``ops.linear`` runs on CPU tensors with ``ops._gpu`` forced true and ``ops.native`` replaced by
a recorder, so every case sees the exact ``C.gemm`` / ``C.awq_dequant`` calls a GPU step would make: the
call sequence, the epilogue code, the exact set of keyword names, the route knobs (``path``, ``waves``,
``splitk``, ``ntb``) and, for tensor-valued keywords, the very object that was passed in. The GEMM tests
on the GPU call ``C.gemm`` with explicit knobs and the kernel tests compare ``ops.linear`` with
tolerances, so a slip in this decision would select another, equally correct kernel and show up only
as a slower benchmark. The case tables are a record of the routing as it is.
"""
from __future__ import annotations

from types import SimpleNamespace

import pytest
import torch

from vgate import ops

N, K = 64, 128
BF16 = torch.bfloat16
MID4 = ops.MID_BASE - 4  # plan code of the medium kernel with 4 waves per block

# keyword names of one C.gemm call
LONG = {"bias", "res", "ws", "waves", "splitk", "ntb", "path", "fault"}  # M > 16
DEC = LONG | {"sk_ws"}                                                   # M <= 16
AWQ = {"awq_scales", "awq_zeros", "group"}
SZP = {"awq_szp"}
DEQ = {"bias", "res", "ws"}                                              # after awq_dequant
QKV = {"positions", "slots", "cos_sin", "k_cache", "v_cache", "hq", "hkv"}
FA = {"fa_block_tables", "fa_context_lens", "fa_query_start", "fa_out", "fa_part_o", "fa_part_ml", "fa_tickets",
      "fa_sync", "fa_part_size", "fa_scale", "fa_dbg_ts"}
NORM_OUT = {"hg_out", "ssp_out", "hg_gamma"}
AR = {"ar_bases", "ar_rank", "ar_fused_off"}


class Recorder:
    """Stands in for the extension: records (name, positional arguments, keywords)."""

    def __init__(self):
        self.calls = []

    def gemm(self, *a, **kw):
        self.calls.append(("gemm", a, kw))

    def awq_dequant(self, *a, **kw):
        self.calls.append(("awq_dequant", a, kw))


@pytest.fixture
def fake(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(ops, "native", lambda: rec)
    monkeypatch.setattr(ops, "_gpu", lambda t: True)
    return rec


def dense(layout="plain", n=N, **attrs):
    lin = ops.Linear(torch.zeros(n, K, dtype=BF16), bias=torch.zeros(n, dtype=BF16), layout=layout)
    lin.wp = torch.zeros(1, dtype=BF16)  # a Linear built on the CPU keeps no packed copy
    for k, v in attrs.items():
        setattr(lin, k, v)
    return lin


def awq(group=128, szp=True, layout="plain", n=N, **attrs):
    G = K // group
    lin = ops.Linear(None, bias=torch.zeros(n, dtype=BF16),
                     awq=dict(qint=torch.zeros(n, K, dtype=torch.int32), scales=torch.ones(G, n), zeros=torch.zeros(G, n),
                              group=group, layout=layout))
    lin.wp = torch.zeros(1, dtype=torch.int32)  # a Linear built on the CPU keeps the dequantised matrix only
    lin.scales, lin.zeros = torch.ones(G, n, dtype=BF16), torch.zeros(G, n, dtype=BF16)
    lin.szp = torch.zeros(1, dtype=BF16) if szp else None
    for k, v in attrs.items():
        setattr(lin, k, v)
    return lin


def run(lin, M, **kw):
    x = torch.zeros(M, K, dtype=BF16)
    return x, ops.linear(x, lin, **kw)


def same(got, want, what):
    """Numbers and flags by value and type, everything else by identity."""
    if isinstance(want, (bool, int, float)):
        assert type(got) is type(want) and got == want, (what, got, want)
    else:
        assert got is want, (what, got, want)


def gemm_call(fake, lin, x, out, keys, epi=0, res=None, dequant=False, **vals):
    """The recorded calls are one gemm (after one awq_dequant if ``dequant``) with exactly ``keys``."""
    assert [c[0] for c in fake.calls] == (["awq_dequant", "gemm"] if dequant else ["gemm"])
    _, a, kw = fake.calls[-1]
    assert set(kw) == set(keys), (sorted(set(kw) ^ set(keys)), "differ")
    assert a[0] is x and a[2:4] == (lin.N, lin.K) and a[4] is out and a[5] == epi and len(a) == 6
    if dequant:
        _, d, dkw = fake.calls[0]
        scratch = ops.reserve_awq_scratch("cpu", lin.N * lin.K)
        assert d[0] is lin.wp and d[1] is lin.scales and d[2] is lin.zeros
        assert d[3:6] == (lin.N, lin.K, lin.group) and not dkw and len(d) == 8
        assert d[6].data_ptr() == scratch.data_ptr() and d[6].numel() == lin.N * lin.K and a[1] is d[6]
    else:
        assert a[1] is lin.wp
    want = dict(bias=lin.bias, res=res, ws=ops.workspace("cpu"), **vals)
    if "sk_ws" in keys:
        want["sk_ws"] = ops.sk_workspace("cpu")
    if "fault" in keys:
        want["fault"] = ops.fault_word("cpu")
    if AWQ <= set(keys):
        want.update(awq_scales=lin.scales, awq_zeros=lin.zeros, group=lin.group)
    if "awq_szp" in keys:
        want["awq_szp"] = lin.szp
    for k, v in want.items():
        same(kw[k], v, k)
    return (fake.calls[0][1], kw) if dequant else kw


def knobs(path=0, waves=0, splitk=0, ntb=0):
    return dict(path=path, waves=waves, splitk=splitk, ntb=ntb)


AR_STUB = SimpleNamespace(bases=torch.zeros(2, dtype=torch.int64), rank=1, fused_off=4096)
SK = (8, 1, 4)          # a Linear.dec_sk plan
DEC_PLAN = dict(dec_waves=2, dec_splitk=1, dec_ntb=2)
KX_PLAN = dict(dec_path=4, dec_waves=8, dec_splitk=3, dec_ntb=0)


def norm_out_bufs(M=4):
    return (torch.zeros(M, N, dtype=BF16), torch.zeros(M * N // 16), torch.ones(N, dtype=BF16))


# ------------------------------------------------------------------ plan-driven dense routes (rows 1-8)
@pytest.mark.parametrize("M", [1, 16])
def test_dense_decode_no_plan(fake, M):
    lin = dense()
    x, out = run(lin, M)
    gemm_call(fake, lin, x, out, DEC, **knobs())
    assert out.shape == (M, N) and out.dtype == BF16


DENSE_DECODE = [  # id, Linear attributes, ops.STREAMK_DECODE, expected knobs
    ("dec_plan", dict(dec_waves=4, dec_splitk=1, dec_ntb=1), False, knobs(0, 4, 1, 1)),
    ("dec_path_kx", KX_PLAN, False, knobs(4, 8, 3, 0)),
    ("dec_sk", dict(dec_sk=SK), False, knobs(3, 8, 1, 4)),
    ("dec_sk_over_dec_plan", dict(dec_sk=SK, **DEC_PLAN), False, knobs(3, 8, 1, 4)),
    ("streamk_default", dict(dec_sk=None), True, knobs(3, 0, 0, 0)),
    ("streamk_default_over_dec_plan", dict(dec_sk=None, **DEC_PLAN), True, knobs(3, 0, 0, 0)),
    ("dec_sk_false_beats_default", dict(dec_sk=False, **DEC_PLAN), True, knobs(0, 2, 1, 2)),
    ("dec_path_beats_dec_sk", dict(dec_sk=SK, **KX_PLAN), False, knobs(4, 8, 3, 0)),
]


@pytest.mark.parametrize("attrs,streamk,want", [c[1:] for c in DENSE_DECODE], ids=[c[0] for c in DENSE_DECODE])
def test_dense_decode_plans(fake, monkeypatch, attrs, streamk, want):
    monkeypatch.setattr(ops, "STREAMK_DECODE", streamk)
    lin = dense(**attrs)
    x, out = run(lin, 4)
    gemm_call(fake, lin, x, out, DEC, **want)


@pytest.mark.parametrize("attrs", [dict(dec_sk=SK, **DEC_PLAN), dict(dec_sk=SK, **KX_PLAN)], ids=["dec_sk", "dec_sk_kx"])
def test_norm_out_keeps_streamk_out(fake, attrs):
    """The stream-K kernel has no RMSNorm hand-off producer; dec_path still applies."""
    lin = dense(**attrs)
    no = norm_out_bufs()
    x, out = run(lin, 4, norm_out=no)
    want = knobs(lin.dec_path, lin.dec_waves, lin.dec_splitk, lin.dec_ntb)
    gemm_call(fake, lin, x, out, DEC | NORM_OUT, hg_out=no[0], ssp_out=no[1], hg_gamma=no[2], **want)


@pytest.mark.parametrize("attrs", [dict(dec_sk=SK, **DEC_PLAN), KX_PLAN], ids=["dec_sk", "dec_path_kx"])
def test_all_reduce_runs_the_tile_kernels(fake, attrs):
    lin = dense(**attrs)
    x, out = run(lin, 4, ar=AR_STUB)
    gemm_call(fake, lin, x, out, DEC | AR, ar_bases=AR_STUB.bases, ar_rank=1, ar_fused_off=4096,
              **knobs(0, lin.dec_waves, lin.dec_splitk, lin.dec_ntb))


@pytest.mark.parametrize("attrs", [dict(dec_sk=SK, **DEC_PLAN), KX_PLAN], ids=["dec_sk", "dec_path_kx"])
def test_row_gather_runs_the_tile_kernels(fake, attrs):
    lin = dense(**attrs)
    idx = torch.tensor([5, 0, 2, 7], dtype=torch.int32)
    x = torch.zeros(9, K, dtype=BF16)
    out = ops.linear(x, lin, row_idx=idx, out_f32=True)
    gemm_call(fake, lin, x, out, DEC | {"row_idx"}, epi=1, row_idx=idx, **knobs(0, lin.dec_waves, lin.dec_splitk, lin.dec_ntb))
    assert out.shape == (4, N) and out.dtype == torch.float32


# ------------------------------------------------------------------ explicit overrides, medium / prefill plans (rows 9-13)
def test_explicit_waves_ignore_the_decode_plan(fake):
    lin = dense(dec_sk=SK, **KX_PLAN)
    x, out = run(lin, 4, waves=2)
    gemm_call(fake, lin, x, out, DEC, **knobs(0, 2, 0, 0))


def test_explicit_splitk_ignores_the_decode_plan(fake):
    lin = dense(dec_sk=SK, **KX_PLAN)
    x, out = run(lin, 4, splitk=3)
    gemm_call(fake, lin, x, out, DEC, **knobs(0, 0, 3, 0))


def test_explicit_path_keeps_streamk_out(fake):
    lin = dense(dec_sk=SK, **DEC_PLAN)
    x, out = run(lin, 4, path=4)
    gemm_call(fake, lin, x, out, DEC, **knobs(4, 2, 1, 2))


PLAN = {48: (MID4, 3), 128: (128, 2)}
DENSE_PLANNED = [  # M, plan, expected knobs
    (17, PLAN, knobs(2, 4, 3, 0)),
    (48, PLAN, knobs(2, 4, 3, 0)),
    (64, PLAN, knobs()),   # a medium row count takes no prefill bucket's plan
    (128, PLAN, knobs(1, 0, 2, 128)),
    (129, PLAN, knobs()),
    (48, {48: ops.MEDIUM_DEFAULT}, knobs()),
    (128, {128: (0, 0)}, knobs()),
    (100, {256: (0, 0), 128: (64, 0)}, knobs()),
    (130, {256: (1024, 3), 128: (64, 0)}, knobs(1, 0, 3, 1024)),
]


@pytest.mark.parametrize("M,plan,want", DENSE_PLANNED, ids=[f"{i}-M{c[0]}" for i, c in enumerate(DENSE_PLANNED)])
def test_dense_prefill_plan(fake, M, plan, want):
    lin = dense(prefill_plan=dict(plan), dec_sk=SK, **KX_PLAN)  # decode plans play no part above 16 rows
    x, out = run(lin, M)
    gemm_call(fake, lin, x, out, LONG, **want)


@pytest.mark.parametrize("kw,want", [(dict(path=1), knobs(path=1)), (dict(waves=-1), knobs(waves=-1)),
                                     (dict(splitk=2), knobs(splitk=2))], ids=["path", "waves", "splitk"])
def test_explicit_knobs_skip_the_prefill_plan(fake, kw, want):
    lin = dense(prefill_plan=dict(PLAN))
    x, out = run(lin, 128, **kw)
    gemm_call(fake, lin, x, out, LONG, **want)


# ------------------------------------------------------------------ AWQ routes (rows 14-20)
def test_awq_decode(fake):
    lin = awq(dec_sk=SK, dec_path=4)  # dense-only plans
    x, out = run(lin, 8)
    gemm_call(fake, lin, x, out, DEC | AWQ | SZP, **knobs())


def test_awq_decode_takes_dec_plan(fake):
    lin = awq(**DEC_PLAN)
    x, out = run(lin, 8)
    gemm_call(fake, lin, x, out, DEC | AWQ | SZP, **knobs(0, 2, 1, 2))


@pytest.mark.parametrize("M", [17, 48, 64])
def test_awq_medium(fake, M):
    lin = awq(prefill_plan=dict(PLAN))  # the int4 medium kernel reads no plan
    x, out = run(lin, M)
    gemm_call(fake, lin, x, out, LONG | AWQ | SZP, **knobs(path=2))


@pytest.mark.parametrize("M", [65, 128])
def test_awq_dequant(fake, M):
    lin = awq()
    res = torch.zeros(M, N, dtype=BF16)
    x, out = run(lin, M, residual=res)
    d, _ = gemm_call(fake, lin, x, out, DEQ, res=res, dequant=True)
    assert d[7] is None


@pytest.mark.parametrize("M,plan_kw", [(65, {}), (128, dict(ntb=128, splitk=2, path=1)), (129, {})])
def test_awq_dequant_with_prefill_plan(fake, M, plan_kw):
    lin = awq(prefill_plan=dict(PLAN))
    x, out = run(lin, M)
    gemm_call(fake, lin, x, out, DEQ | set(plan_kw), dequant=True, **plan_kw)


def test_awq_dequant_takes_medium_plan(fake):
    lin = awq(szp=False, prefill_plan=dict(PLAN))
    x, out = run(lin, 48)
    gemm_call(fake, lin, x, out, DEQ | {"path", "waves", "splitk"}, dequant=True, path=2, waves=4, splitk=3)


NO_MID = [("no_szp", dict(szp=False), AWQ), ("group64", dict(group=64, szp=False), AWQ),
          ("group64_szp", dict(group=64), AWQ | SZP)]


@pytest.mark.parametrize("kw,keys", [c[1:] for c in NO_MID], ids=[c[0] for c in NO_MID])
def test_awq_without_medium_kernel(fake, kw, keys):
    """No packed (scale, zero) operand or group 64: 17 rows are below AWQ_DEQUANT_MIN_M, 48 dequantise."""
    lin = awq(**kw)
    x, out = run(lin, 17)
    gemm_call(fake, lin, x, out, LONG | keys, **knobs())
    fake.calls.clear()
    x, out = run(lin, 48)
    gemm_call(fake, lin, x, out, DEQ, dequant=True)


def test_awq_dequant_threshold_is_read_at_call_time(fake, monkeypatch):
    monkeypatch.setattr(ops, "AWQ_DEQUANT_MIN_M", 17)
    lin = awq(szp=False)
    x, out = run(lin, 17)
    gemm_call(fake, lin, x, out, DEQ, dequant=True)


def test_awq_explicit_waves_pass_through(fake):
    lin = awq()
    x, out = run(lin, 48, waves=4)
    gemm_call(fake, lin, x, out, LONG | AWQ | SZP, **knobs(waves=4))


def test_awq_explicit_path_still_dequantises(fake):
    """The dequant branch does not look at ``path``."""
    lin = awq()
    x, out = run(lin, 100, path=1)
    gemm_call(fake, lin, x, out, DEQ, dequant=True)


def test_awq_row_gather_stays_int4(fake):
    lin = awq()
    idx = torch.arange(48, dtype=torch.int32)
    x = torch.zeros(48, K, dtype=BF16)
    out = ops.linear(x, lin, row_idx=idx, out_f32=True)
    gemm_call(fake, lin, x, out, LONG | AWQ | SZP | {"row_idx"}, epi=1, row_idx=idx, **knobs())


# ------------------------------------------------------------------ norm, qkv, fused attention, all-reduce (rows 21-27)
def test_norm_folded_gamma(fake):
    lin = dense(norm_gamma=torch.ones(K))
    w = torch.ones(K, dtype=BF16)
    x, out = run(lin, 4, norm=(w, 1e-5))
    gemm_call(fake, lin, x, out, DEC | {"rownorm", "eps"}, rownorm=True, eps=1e-5, **knobs())


def test_norm_weight(fake):
    lin = dense()
    w = torch.ones(K, dtype=BF16)
    x, out = run(lin, 4, norm=(w, 1e-5))
    gemm_call(fake, lin, x, out, DEC | {"norm_w", "eps"}, norm_w=w, eps=1e-5, **knobs())


def test_prenorm(fake):
    lin = awq()
    ssp = torch.zeros(4 * K // 16)
    x, out = run(lin, 4, prenorm=(ssp, 1e-6))
    gemm_call(fake, lin, x, out, DEC | AWQ | SZP | {"ssp_in", "eps"}, ssp_in=ssp, eps=1e-6, **knobs())


@pytest.mark.parametrize("gamma", [False, True])
def test_awq_dequant_norm_and_qkv(fake, gamma):
    """The dequantised matrix carries gamma, so the bf16 kernels get the row-scale mode whatever norm_gamma says."""
    lin = awq(layout="qkv", n=384)
    if gamma:
        lin.norm_gamma = torch.ones(K)
    w = torch.ones(K, dtype=BF16)
    q = qkv_args(128)
    x, out = run(lin, 128, norm=(w, 1e-5), qkv=q)
    d, _ = gemm_call(fake, lin, x, out, DEQ | {"rownorm", "eps"} | QKV, epi=3, dequant=True, rownorm=True, eps=1e-5, **q)
    assert d[7] is w and out.shape == (128, 128)


def qkv_args(M):
    return dict(positions=torch.zeros(M, dtype=torch.int32), slots=torch.zeros(M, dtype=torch.int32),
                cos_sin=torch.zeros(8, 128), k_cache=torch.zeros(2, 1, 16, 128, dtype=BF16),
                v_cache=torch.zeros(2, 1, 16, 128, dtype=BF16), hq=1, hkv=1)


def attn_args():
    e = torch.zeros(4, dtype=torch.int32)
    return dict(block_tables=e.clone(), context_lens=e.clone(), query_start=e.clone(), out=torch.zeros(4, 128, dtype=BF16),
                part_o=torch.zeros(4), part_ml=torch.zeros(4), part_size=256, scale=0.125)


def fa_values(a):
    return dict(fa_block_tables=a["block_tables"], fa_context_lens=a["context_lens"], fa_query_start=a["query_start"],
                fa_out=a["out"], fa_part_o=a["part_o"], fa_part_ml=a["part_ml"], fa_tickets=ops.attn_tickets("cpu"),
                fa_sync=ops.qa_sync("cpu"), fa_part_size=256, fa_scale=0.125, fa_dbg_ts=None)


def test_silu_epilogue(fake):
    lin = dense(layout="silu")
    x, out = run(lin, 4)
    gemm_call(fake, lin, x, out, DEC, epi=2, **knobs())
    assert out.shape == (4, N // 2)


def test_qkv_fused_attention(fake):
    lin = dense(layout="qkv", n=384)
    q, a = qkv_args(4), attn_args()
    x, out = run(lin, 4, qkv=q, attn=a)
    gemm_call(fake, lin, x, out, DEC | QKV | FA, epi=3, **q, **fa_values(a), **knobs())
    assert out.shape == (4, 128)


def test_qkv_attention_in_two_launches(fake, monkeypatch):
    after = []
    monkeypatch.setattr(ops, "FUSE_QKV_ATTN", False)
    monkeypatch.setattr(ops, "_attn_after", lambda *args: after.append(args))
    lin = dense(layout="qkv", n=384)
    q, a = qkv_args(4), attn_args()
    x, out = run(lin, 4, qkv=q, attn=a)
    gemm_call(fake, lin, x, out, DEC | QKV, epi=3, **q, **knobs())
    assert len(after) == 1 and after[0][0] is out and after[0][1] is q and after[0][2] is a


def test_attention_needs_the_decode_qkv_projection(fake):
    with pytest.raises(ValueError, match="fused attention"):
        run(dense(), 4, attn=attn_args())
    with pytest.raises(ValueError, match="fused attention"):
        run(dense(layout="qkv", n=384), 17, qkv=qkv_args(17), attn=attn_args())
    assert fake.calls == []


def test_all_reduce_needs_decode_rows_and_bf16(fake):
    with pytest.raises(ValueError, match="fused all-reduce"):
        run(dense(), 17, ar=AR_STUB)
    with pytest.raises(ValueError, match="fused all-reduce"):
        run(dense(), 4, ar=AR_STUB, out_f32=True)
    assert fake.calls == []
