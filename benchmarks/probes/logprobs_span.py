"""Cost of a logprob step on the MI355X (csrc/kernels/logprobs.hip) beside the sampler it follows.

    python benchmarks/probes/logprobs_span.py [--vocab 151936] [--rows 8] [--k 5 20]

One captured graph per k holds what a decode step runs on its logits: the sampler (T 0.7, top-p 0.9)
and the two logprob launches, with the launch timeline on. Per kernel it reports the block span
(first block start -> last block end, median / min of 21 replays, from the in-kernel stamps) and the
replayed time per step with and without the logprob launches. The last line is the host time a
logprob step adds to ``ModelRunner.launch()``: the runner's own ``_launch_logprobs`` (k_rows upload,
two launches, record download) enqueued 200 times on a tiny engine's runner over logits of this
shape, the device drained every 20 calls so the queue never back-pressures the host.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import torch  # noqa: E402

from vgate import ops  # noqa: E402


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _replay_us(g, reps=20):
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--k", type=int, nargs="+", default=[5, 20])
    a = ap.parse_args()
    C = ops.native()
    dev = "cuda"
    S, V = a.rows, a.vocab
    g0 = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(S, V, device=dev, generator=g0) * 4
    temp = torch.full((S,), 0.7, device=dev)
    topp = torch.full((S,), 0.9, device=dev)
    topk = torch.full((S,), -1, dtype=torch.int32, device=dev)
    seeds = torch.arange(S, dtype=torch.int64, device=dev)
    offs = torch.zeros(S, dtype=torch.int64, device=dev)
    toks = torch.zeros((S + 3) // 4 * 4, dtype=torch.int32, device=dev)
    rec = torch.zeros(S, ops.LOGPROB_REC_WORDS, dtype=torch.int32, device=dev)

    def sampler():
        ops.sample(logits, temp, topp, topk, seeds, offs, out=toks[:S])

    sampler()
    ops.logprobs(logits, toks, torch.zeros(S, dtype=torch.int32, device=dev), out=rec)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    plain = torch.cuda.CUDAGraph()
    with torch.cuda.graph(plain, stream=side):
        sampler()
    torch.cuda.current_stream().wait_stream(side)
    plain_us = _replay_us(plain)
    for k in a.k:
        k_rows = torch.full((S,), k, dtype=torch.int32, device=dev)
        buf = torch.zeros(1 << 14, dtype=torch.int64, device=dev)
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        C.timeline_start(buf)
        with torch.cuda.graph(g, stream=side):
            sampler()
            ops.logprobs(logits, toks, k_rows, out=rec)
        C.timeline_stop()
        entries = C.timeline_entries()  # (kernel, offset, blocks) per captured launch
        torch.cuda.current_stream().wait_stream(side)
        spans = {name: [] for name, _, _ in entries}
        both = []
        for _ in range(21):
            buf.zero_()
            g.replay()
            torch.cuda.synchronize()
            t = buf.cpu()
            lo, hi = None, None
            for name, off, blocks in entries:
                st = t[off: off + 2 * blocks].view(-1, 2)
                spans[name].append(float(st[:, 1].max() - st[:, 0].min()) / 100.0)  # 100 MHz clock -> us
                if name.startswith("logprob"):
                    lo = st[:, 0].min() if lo is None else min(lo, st[:, 0].min())
                    hi = st[:, 1].max() if hi is None else max(hi, st[:, 1].max())
            both.append(float(hi - lo) / 100.0)
        out = {"vocab": V, "rows": S, "k": k, "segments": C.logprob_segments(S, V),
               "sampler_segments": C.sample_segments(S, V)}
        for name, xs in spans.items():
            out[f"{name}_span_us_median"] = round(_median(xs), 2)
            out[f"{name}_span_us_min"] = round(min(xs), 2)
        out["logprob_part_to_merge_end_us_median"] = round(_median(both), 2)
        out["graph_us_sampler_only"] = round(plain_us, 2)
        out["graph_us_sampler_and_logprobs"] = round(_replay_us(g), 2)
        print(json.dumps(out), flush=True)

    # host time of the runner's logprob step (its real code path), on logits of this shape
    from vgate.runtime.engine import EngineConfig, LLMEngine
    eng = LLMEngine(EngineConfig(model="tiny", device="cuda", max_model_len=128, max_num_seqs=max(S, 8),
                                 max_num_batched_tokens=64, num_kv_blocks=32, warmup=False))
    r = eng.runner
    rows = {s: a.k[0] for s in range(S)}
    with torch.inference_mode():
        r._launch_logprobs(logits, rows, S, 0)
        torch.cuda.synchronize()
        host = []
        for i in range(200):
            t0 = time.perf_counter()
            r._launch_logprobs(logits, rows, S, i & 1)
            host.append(1e6 * (time.perf_counter() - t0))
            if i % 20 == 19:
                torch.cuda.synchronize()
        t0 = time.perf_counter()
        ent = r._lp_entries(rows, 1)
        parse_us = 1e6 * (time.perf_counter() - t0)
    assert len(ent) == S and all(len(e[2]) == a.k[0] for e in ent.values())
    print(json.dumps({"rows": S, "k": a.k[0], "launch_host_us_median": round(_median(host), 1),
                      "launch_host_us_p90": round(sorted(host)[180], 1),
                      "collect_parse_us": round(parse_us, 1)}), flush=True)


if __name__ == "__main__":
    main()
