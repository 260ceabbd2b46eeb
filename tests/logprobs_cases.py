"""Shared cases of the logprob tests: one padded logits buffer per (V, S) with every row kind and
chosen-token position of the kernels' edge cases, and its float64 reference, built once."""
import functools
import math
from dataclasses import dataclass

import torch

from vgate.ops import reference as ref

GUARD = 1e30  # columns [V, ldl) of the padded buffer: never a candidate, never in the sum
KS = (20, 5, -1, 1, 0)  # per-row k, by row index
KINDS = ("gauss1", "gauss20", "plus80", "minus80", "ties", "neginf")


def segments(S: int, V: int) -> int:
    """The launcher's segments per row (csrc/kernels/logprobs.hip logprob_segments)."""
    if S > 128:
        return 1
    return max(1, min(256 // S, 32, ((V + 3) // 4) // 256))


def row_kind(r: int, S: int) -> str:
    return KINDS[(r + S) % len(KINDS)]


@dataclass
class Case:
    V: int
    S: int
    ldl: int
    buf: torch.Tensor      # [S, ldl] fp32 (CPU): logits, then GUARD columns
    tokens: torch.Tensor   # [S] int32, some outside [0, V) (the kernel clamps)
    k_rows: torch.Tensor   # [S] int32
    chosen: torch.Tensor   # reference (float64 / int64), left unchanged by the tests
    top_ids: torch.Tensor
    top_lp: torch.Tensor


@functools.lru_cache(maxsize=None)
def build_case(V: int, S: int, seed: int = 0) -> Case:
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + S)
    ldl = (V + 3) // 4 * 4 + 64
    buf = torch.full((S, ldl), GUARD, dtype=torch.float32)
    nseg = segments(S, V)
    V4 = (V + 3) // 4
    mid = nseg // 2
    first_mid = 4 * (V4 * mid // nseg)
    last_mid = min(V, 4 * (V4 * (mid + 1) // nseg)) - 1
    tokens = torch.zeros(S, dtype=torch.int32)
    k_rows = torch.zeros(S, dtype=torch.int32)
    for r in range(S):
        kind = row_kind(r, S)
        x = torch.randn(V, generator=g)
        if kind == "gauss20":
            x = x * 20
        elif kind == "plus80":
            x = x + 80
        elif kind == "minus80":
            x = x - 80
        elif kind == "ties":  # quarters: ties everywhere, across segment and wave boundaries
            x = torch.randint(-8, 8, (V,), generator=g).float() / 4
        elif kind == "neginf":
            idx = torch.randperm(V, generator=g)[: min(50, V // 2)]
            x[idx] = float("-inf")
        buf[r, :V] = x
        tokens[r] = (0, V - 1, first_mid, last_mid, int(torch.randint(0, V, (1,), generator=g)), V + 5, -3)[r % 7]
        k_rows[r] = KS[r % len(KS)]
        if kind == "neginf" and r % 2:  # a chosen token of probability zero
            tokens[r] = int(idx[0])
    chosen, top_ids, top_lp = ref.logprobs_ref(buf[:, :V], tokens, k_rows)
    return Case(V, S, ldl, buf, tokens, k_rows, chosen, top_ids, top_lp)


def check_entries(seq, k):
    """The internal consistency of a greedy request's entries (shared with the GPU engine tests)."""
    assert len(seq.logprobs) == len(seq.output_ids)
    for tok, (tid, lp, top) in zip(seq.output_ids, seq.logprobs):
        assert tid == tok and len(top) == k
        assert top[0] == (tid, lp)  # greedy: the chosen token is the most likely one
        vals = [v for _, v in top]
        assert all(a >= b for a, b in zip(vals, vals[1:]))
        assert sum(math.exp(v) for v in vals) <= 1 + 1e-6
        assert len({t for t, _ in top}) == k
