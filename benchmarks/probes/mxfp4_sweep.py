"""MXFP4 (e2m1 W4A16) against FP8 (e4m3 W8A16) and bf16 per layer shape on the MI355X, cold weights.

Decode: the mxfp4 decode kernel (csrc/kernels/gemm_mxfp4.hip) and the fp8 decode kernel against the dense
bf16 decode path of the same shape with its measured decode plan (vgate/models/decode_plans.py),
Qwen2.5-1.5B and Llama-3-8B layer shapes at M = 1, 8, 16, each projection with the epilogue and fused
RMSNorm it has in the model. Prefill: the 448-row dequant + bf16 GEMM pair against the bf16 GEMM alone.
Every launch is timed by events with the Infinity Cache flushed first (a 512 MiB read sweep, as the
start-up tuner's cold timer does); the figure is the median over ``--iters`` launches and includes the
event pair's own overhead, the same on every side. ``--ntb 1,2,4`` also times the mxfp4 kernel with that
many 16-column tiles per block forced (``mxfp4_ntbN_us``); ``--plan-sweep`` times every (waves, K slices,
tiles per block) of PLAN_GRID on the mxfp4 kernel and reports the three fastest beside the launcher's own
plan (``mxfp4_plans``: the data behind the mxfp4 entries of vgate/models/decode_plans.py).

    python benchmarks/probes/mxfp4_sweep.py [--sides bf16,fp8,mxfp4] [--iters 30] [--models qwen,llama]

``--sides bf16`` uses nothing of the quantized paths, so the same file times the bf16 side on an older tree.
Prints one JSON line per (model, projection, M).
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import torch  # noqa: E402

from vgate import ops  # noqa: E402
from vgate.models import decode_plans  # noqa: E402
from vgate.ops.tuner import _event_ms  # noqa: E402

# (projection, N, K, layout, (hq, hkv), norm fused in, residual)
MODELS = {
    "qwen2.5-1.5b": [("qkv", 2048, 1536, "qkv", (12, 2), True, False), ("o", 1536, 1536, "plain", None, False, True),
                     ("gate_up", 17920, 1536, "silu", None, True, False), ("down", 1536, 8960, "plain", None, False, True)],
    "llama-3-8b": [("qkv", 6144, 4096, "qkv", (32, 8), True, False), ("o", 4096, 4096, "plain", None, False, True),
                   ("gate_up", 28672, 4096, "silu", None, True, False), ("down", 4096, 14336, "plain", None, False, True)],
}


def apply_plan(lin):
    """decode_plans.apply for one Linear."""
    p = decode_plans.lookup(lin)
    if p is None:
        return
    if p[0] == "sk":
        lin.dec_sk = tuple(p[1:])
    elif p[0] == "kx":
        lin.dec_path = ops.PATH_KX
        lin.dec_waves, lin.dec_splitk, lin.dec_ntb = p[1:]
    else:
        lin.dec_waves, lin.dec_splitk, lin.dec_ntb = p


def cold_median_us(run, iters: int, flush: torch.Tensor) -> float:
    """Median device time of one launch, the Infinity Cache flushed before each."""
    C = ops.native()
    ts = []
    for _ in range(iters):
        C.prefetch(flush, 1024)
        ts.append(_event_ms(run))
    return 1e3 * sorted(ts)[len(ts) // 2]


PLAN_GRID = [(w, s, t) for w in (2, 4, 8) for s in (1, 2, 4) for t in (1, 2, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="bf16,fp8,mxfp4")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--models", default="qwen,llama")
    ap.add_argument("--ms", default="1,8,16,448")
    ap.add_argument("--ntb", default="", help="also time the mxfp4 decode kernel with these tiles per block forced")
    ap.add_argument("--plan-sweep", action="store_true", help="time PLAN_GRID on the mxfp4 decode kernel")
    a = ap.parse_args()
    dev = torch.device("cuda")
    flush = torch.empty(512 * 2**20, dtype=torch.uint8, device=dev)
    sides = a.sides.split(",")
    ntbs = [int(v) for v in a.ntb.split(",") if v]
    ms = [int(m) for m in a.ms.split(",")]
    for model, shapes in MODELS.items():
        if not any(model.startswith(m) for m in a.models.split(",")):
            continue
        for name, N, K, layout, heads, normed, resid in shapes:
            g = torch.Generator(device=dev)
            g.manual_seed(N + K)
            w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).bfloat16()
            lins = {}
            if "bf16" in sides:
                lins["bf16"] = ops.Linear(w, layout=layout)
                if normed:
                    lins["bf16"].fold_norm(torch.ones(K, dtype=torch.bfloat16, device=dev))
                apply_plan(lins["bf16"])
            if "fp8" in sides:
                lins["fp8"] = ops.Linear.quantize_fp8(w, layout=layout)
            if "mxfp4" in sides:
                lins["mxfp4"] = ops.Linear.quantize_mxfp4(w, layout=layout)
                if not a.plan_sweep and not ntbs:  # as in the model; the --ntb / --plan-sweep baselines are the launcher's own plan
                    apply_plan(lins["mxfp4"])
            del w
            gamma = torch.ones(K, dtype=torch.bfloat16, device=dev)
            for M in ms:
                x = torch.randn(M, K, device=dev, generator=g).bfloat16()
                ncols = N // 2 if layout == "silu" else heads[0] * 128 if heads else N
                out = torch.zeros(M, ncols, dtype=torch.bfloat16, device=dev)
                qkv = None
                if heads:
                    hq, hkv = heads
                    nblk = (M + 15) // 16 + 1
                    qkv = dict(positions=torch.arange(M, dtype=torch.int32, device=dev),
                               slots=torch.arange(M, dtype=torch.int32, device=dev),
                               cos_sin=ops.ref.rope_cos_sin(max(M, 16) + 1, 128, 1e6, device=dev),
                               k_cache=torch.zeros(nblk, hkv, 16, 128, dtype=torch.bfloat16, device=dev),
                               v_cache=torch.zeros(nblk, hkv, 16, 128, dtype=torch.bfloat16, device=dev), hq=hq, hkv=hkv)
                row = {"model": model, "proj": name, "N": N, "K": K, "M": M}
                for side, lin in lins.items():
                    kw = dict(out=out, qkv=qkv, norm=(gamma, 1e-6) if normed else None,
                              residual=out if resid else None)

                    def run():
                        ops.linear(x, lin, **kw)
                    run()
                    torch.cuda.synchronize()
                    us = cold_median_us(run, a.iters, flush)
                    row[side + "_us"] = round(us, 2)
                    row[side + "_TBps"] = round(lin.nbytes() / us / 1e6, 2)
                    if side == "mxfp4" and M <= 16:
                        for nt in ntbs:
                            lin.dec_ntb = nt
                            run()
                            row[f"mxfp4_ntb{nt}_us"] = round(cold_median_us(run, a.iters, flush), 2)
                        lin.dec_ntb = 0
                        if a.plan_sweep:
                            got = []
                            for w_, s_, t_ in PLAN_GRID:
                                if layout == "qkv" and t_ != 1:
                                    continue
                                lin.dec_waves, lin.dec_splitk, lin.dec_ntb = w_, s_, t_
                                run()
                                got.append((round(cold_median_us(run, a.iters, flush), 2), w_, s_, t_))
                            lin.dec_waves = lin.dec_splitk = lin.dec_ntb = 0
                            row["mxfp4_plans"] = sorted(got)[:3]
                for side in ("fp8", "mxfp4"):
                    if side in lins and "bf16" in lins:
                        row[side + "_over_bf16"] = round(row[side + "_us"] / row["bf16_us"], 3)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
