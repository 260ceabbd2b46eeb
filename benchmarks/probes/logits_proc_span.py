"""Span of the logits-processor kernel alone (csrc/kernels/logits_proc.hip) on the MI355X.

    python benchmarks/probes/logits_proc_span.py [--vocab 151936] [--rows 8] [--entries 100 2100]

Per entry count: rows x entries unique-token entries packed through the engine's own host state
(SeqProcState -> ProcMeta), half of the rows with an in-flight token. Reports the block span of one
launch from the in-kernel timeline stamps (first block start -> last block end, median of 21
launches) and the time per launch of a captured graph of 50 launches replayed back to back.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vgate import ops  # noqa: E402
from vgate.runtime.logits_proc import ProcMeta, SeqProcState  # noqa: E402
from vgate.runtime.sampling_params import SamplingParams  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--entries", type=int, nargs="+", default=[100, 2100])
    a = ap.parse_args()
    C = ops.native()
    dev = "cuda"
    rng = np.random.default_rng(0)
    S, V = a.rows, a.vocab
    sp = SamplingParams(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.5)
    logits = torch.randn(S, V, device=dev)
    prev = torch.randint(0, V, (S + 3,), dtype=torch.int32, device=dev)
    pm = ProcMeta(S, V, 4096, dev)
    for n in a.entries:
        rows = []
        for s in range(S):
            toks = rng.permutation(V)[:n].tolist()
            st = SeqProcState(toks[: n // 2])
            for t in toks[n // 2:]:
                st.add_output(t)
            rows.append((st, sp, -(s + 1) if s % 2 else 0))
        used = pm.fill(0, rows, S)
        pm.upload(0)
        pv = pm.view(S)
        ops.process_logits(logits, pv, prev)
        torch.cuda.synchronize()
        spans = []
        for _ in range(21):
            buf = torch.zeros(1 << 12, dtype=torch.int64, device=dev)
            C.timeline_start(buf)
            ops.process_logits(logits, pv, prev)
            nstamp = C.timeline_stop()
            torch.cuda.synchronize()
            t = buf[:nstamp].view(-1, 2).cpu()
            spans.append(float(t[:, 1].max() - t[:, 0].min()) / 100.0)  # 100 MHz clock -> us
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(50):
                ops.process_logits(logits, pv, prev)
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({"vocab": V, "rows": S, "entries_per_row": n, "entries": used,
                          "uploaded_bytes": pm.header_bytes + 16 * used,
                          "block_span_us_median": round(sorted(spans)[len(spans) // 2], 2),
                          "block_span_us_min": round(min(spans), 2),
                          "graph_us_per_launch": round(1e3 * e0.elapsed_time(e1) / 500, 2)}), flush=True)
        logits.normal_()


if __name__ == "__main__":
    main()
