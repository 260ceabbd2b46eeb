"""qk_norm_rope_kv against rope_kv on the same shapes (MI355X): the new kernel moves the same bytes as the
RoPE + KV-write kernel (qkv row in, q and the two cache rows out; + 512 B of norm weights), so rope_kv's time
is its yardstick.

Per shape (T = 8 and T = 448, Hq = 16, Hkv = 8: Qwen3-0.6B / 1.7B), both kernels alternating, ROUNDS times:
  warm : a captured graph of REPS back-to-back launches, device events around one replay, / REPS
  cold : one launch behind a 512 MiB read sweep (the Infinity Cache flushed), device events around the launch
         alone (this figure includes the event pair's own few us, the same for both kernels)
Prints one JSON line with the medians, the min..max spread over the rounds and the ratios.

    python benchmarks/probes/qk_norm_probe.py
"""
from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import torch  # noqa: E402

from vgate import ops  # noqa: E402

REPS, ROUNDS, COLD_ITERS = 200, 7, 10


def _ms(run) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    C = ops.native()
    dev = torch.device("cuda")
    Hq, Hkv, D = 16, 8, 128
    flush = torch.empty(512 * 2**20, dtype=torch.uint8, device=dev)
    cos_sin = ops.ref.rope_cos_sin(4096, D, 1e6, device=dev)
    qn = (0.5 + 3.5 * torch.rand(D, device=dev)).bfloat16()
    kn = (0.5 + 3.5 * torch.rand(D, device=dev)).bfloat16()
    res = {}
    for T in (8, 448):
        qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=dev).bfloat16()
        kc = torch.zeros(4096, Hkv, 16, D, device=dev, dtype=torch.bfloat16)
        vc = torch.zeros_like(kc)
        pos = (torch.arange(T, dtype=torch.int32, device=dev) * 7 + 40) % 4096
        slots = (torch.arange(T, dtype=torch.int32, device=dev) * 16 * 37 + 3) % (4096 * 16)
        q_out = torch.empty(T, Hq * D, device=dev, dtype=torch.bfloat16)
        kernels = {
            "rope_kv": lambda: C.rope_kv(qkv, pos, slots, cos_sin, kc, vc, Hq, Hkv, D, q_out),
            "qk_norm_rope_kv": lambda: C.qk_norm_rope_kv(qkv, pos, slots, cos_sin, qn, kn, 1e-6, kc, vc, Hq, Hkv,
                                                         q_out),
        }
        graphs = {}
        for name, fn in kernels.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(REPS):
                    fn()
            g.replay()
            torch.cuda.synchronize()
            graphs[name] = g
        warm = {k: [] for k in kernels}
        cold = {k: [] for k in kernels}
        for _ in range(ROUNDS):
            for name, fn in kernels.items():  # alternating
                warm[name].append(_ms(graphs[name].replay) * 1e3 / REPS)
                tot = 0.0
                for _ in range(COLD_ITERS):
                    C.prefetch(flush, 1024)
                    tot += _ms(fn)
                cold[name].append(tot * 1e3 / COLD_ITERS)
        row = {}
        for mode, d in (("warm", warm), ("cold", cold)):
            for name, v in d.items():
                row[f"{mode}_{name}_us"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                            "max": round(max(v), 3)}
            row[f"{mode}_ratio"] = round(statistics.median(d["qk_norm_rope_kv"]) / statistics.median(d["rope_kv"]), 3)
        res[f"T={T}"] = row
    print(json.dumps({"qk_norm_probe": {"Hq": Hq, "Hkv": Hkv, "reps": REPS, "rounds": ROUNDS, **res}}), flush=True)


if __name__ == "__main__":
    main()
