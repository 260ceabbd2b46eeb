"""Measured decode-GEMM decompositions (M <= 16) per weight shape, applied to every matching
Linear at model construction (``Linear.dec_waves / dec_splitk / dec_ntb``; 0 = the launcher's
heuristic, csrc/kernels/gemm_decode.h ``plan``).

Entries come from in-context sweeps: every candidate (waves per block, K slices, column tiles
per block) re-captures the decode hipGraph and times the WHOLE step, all other projections at
their current plan (benchmarks/decode_sweep.py for TP = 1 models, benchmarks/tp_rank_bench.py
--sweep for one TP rank's shapes). A shape missing here measured best on the heuristic.

Key: (N, K, layout, weight kind) of the packed weight; layout "qkv" / "silu" / "plain".
Value: (waves, K slices, column tiles per block) of the tile-per-block kernels, ("kx", waves, K
slices, tiles code) for the register-stationary kernel (PATH_KX; 0 = its own grid rule), or
("sk", waves, blocks per CU, k-steps per register group) for the stream-K kernel
(csrc/kernels/gemm_streamk.hip: one equal share of the weight stream per CU), which wins on the
large matrices where the tile count leaves CUs uneven (benchmarks/probes/sk_probe.py,
profiles/r4_streamk_probe.log).
"""
from __future__ import annotations

from vgate.ops import PATH_KX

PLANS: dict[tuple[int, int, str, str], tuple] = {
    # Llama-3-70B TP = 8, one rank, batch 8, ctx 128: round-5 in-context sweep with the register-stationary
    # and stream-K candidates (profiles/r5_tp8_rank_sweep.log; round 3: profiles/r3_tp8_rank_sweep.log)
    (1280, 8192, "qkv", "dense"): ("kx", 8, 3, 0),  # 80 tiles x 3 K slices, 8 waves (tile kernel 8 x 3: +56 us)
    (8192, 1024, "plain", "dense"): ("kx", 0, 1, 0),  # o_proj: 512 one-tile blocks (tile kernel 2 x 1: +13 us)
    (7168, 8192, "silu", "dense"): (4, 1, 0),    # gate_up: 448 one-tile blocks at 4 waves (heuristic 8: +67 us)
    # down_proj (8192, 3584): the heuristic tile plan (stream-K 4 x 1 x 8, the round-4 entry: +94 us since the
    # round-5 wait fixes). A rank with the fused row-parallel all-reduce (the TP default) runs o / down on
    # the tile kernels with the all-reduce epilogue whatever the entry says (vgate/ops linear: path 0 with ar)
    (16032, 8192, "plain", "dense"): (8, 1, 1),  # LM head shard
    # Llama-3-8B, batch 8 (r4 probe, profiles/r4_streamk_probe.log): qkv on stream-K (13.6 vs 15.1 us per
    # launch); gate_up and down_proj on 4-wave tile blocks (39.0 vs 41.3, 21.1 vs 21.9 us)
    (6144, 4096, "qkv", "dense"): ("sk", 8, 1, 4),
    (28672, 4096, "silu", "dense"): (4, 1, 0),
    (4096, 14336, "plain", "dense"): (4, 1, 1),
    # Qwen2.5-1.5B bf16 gate_up on the register-stationary kernel (one block per CU owning 4-5 whole
    # tiles, every weight fragment requested at once; csrc/kernels/gemm_kx.h): 10.5 vs 11.9 us per
    # launch as the hand-off consumer, cold weights (benchmarks/probes/dense_kx_sweep.py,
    # profiles/r5_dense_kx_sweep.log). qkv / o_proj / down_proj stay on the tile kernels there.
    (17920, 1536, "silu", "dense"): ("kx", 0, 0, 0),
    # Qwen2.5-1.5B AWQ int4: no entries — every int4 decode GEMM runs the register-stationary kernel
    # (csrc/kernels/gemm_kx.h / gemm_kx_q4.hip) on its own grid rule (round 3's awq_stream / wide plans:
    # profiles/r3_awq_decode_sweep.log)
}

# MXFP4 (csrc/kernels/gemm_mxfp4.hip): the same key and value forms as PLANS, in a table of its own (PLANS holds
# the dense and AWQ kinds only). Unlike the entries above these come from the per-launch cold-weight
# probe, not a whole-step sweep (benchmarks/probes/mxfp4_sweep.py --plan-sweep, profiles/mxfp4_plan_sweep.log;
# us at M = 8, the launcher's own plan first): at 4 bits a wave's weight stream is a quarter of the bf16
# one, so the large matrices want more K slices or tile groups in flight than the bf16 heuristic gives.
# o_proj of both models and the Qwen qkv measured best on the heuristic.
MXFP4_PLANS: dict[tuple[int, int, str, str], tuple] = {
    (17920, 1536, "silu", "mxfp4"): (4, 1, 4),   # Qwen2.5-1.5B gate_up: 15.5 -> 14.5
    (1536, 8960, "plain", "mxfp4"): (4, 4, 2),   # Qwen2.5-1.5B down: 13.4 -> 11.5 (M = 16: 17.2 -> 12.1)
    (6144, 4096, "qkv", "mxfp4"): (4, 2, 1),     # Llama-3-8B qkv: 18.1 -> 15.7
    (28672, 4096, "silu", "mxfp4"): (4, 1, 4),   # Llama-3-8B gate_up: 31.6 -> 24.4
    (4096, 14336, "plain", "mxfp4"): (8, 4, 4),  # Llama-3-8B down: 17.4 -> 15.1 (M = 16: 22.8 -> 16.8; later runs 20.2 / 25.0: README "MXFP4")
}


def lookup(lin):
    """The measured plan of one Linear, or None."""
    key = (lin.N, lin.K, lin.layout, lin.kind)
    return PLANS.get(key) or MXFP4_PLANS.get(key)


def apply(model) -> int:
    """Set the measured plan on every Linear of ``model`` whose shape has one; returns how many."""
    n = 0
    lins = [lin for L in model.layers for lin in (L.qkv, L.o, L.gate_up, L.down)] + [model.lm_head]
    for lin in lins:
        p = lookup(lin)
        if p is not None:
            if p[0] == "sk":
                lin.dec_sk = tuple(p[1:])
            elif p[0] == "kx":
                lin.dec_path = PATH_KX
                lin.dec_waves, lin.dec_splitk, lin.dec_ntb = p[1:]
            else:
                lin.dec_waves, lin.dec_splitk, lin.dec_ntb = p
            n += 1
    return n
