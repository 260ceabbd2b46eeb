"""Case builder shared by tests/test_logits_proc_cpu.py and tests/test_logits_proc_gpu.py: random
token histories with a chosen number of unique-token entries, packed through the engine's own host
state (SeqProcState -> ProcMeta), and the expected rows from the dense oracle
(vgate.ops.reference.process_logits_ref), which knows nothing of the sparse encoding."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from vgate.ops import reference as ref
from vgate.runtime.logits_proc import ProcMeta, SeqProcState
from vgate.runtime.sampling_params import SamplingParams

# (repetition, presence, frequency): rep below / at / above 1, negative pres and freq included
PARAMS = [(1.3, 0.7, 0.4), (0.5, -0.6, -0.3), (1.0, 0.25, 1.5), (1.3, 0.0, 0.0), (1.0, 0.0, 0.0)]
PENDING = ("hist", "bias", "none", "absent")


@dataclass
class Row:
    prompt: list
    outputs: list          # every generated token, the in-flight one (pending) last
    params: SamplingParams
    state: SeqProcState | None
    pend_tok: int | None   # the in-flight token, None = nothing pending


def make_row(rng, V: int, n: int, pending: str, par: tuple, oob: bool = False, edge: bool = True) -> Row:
    """A history whose host state holds exactly ``n`` in-range unique tokens before the in-flight
    token is counted. ``pending``: the in-flight token equals a token with history ("hist"), a
    bias-only token ("bias"), no entry at all ("none"), or there is none ("absent")."""
    perm = rng.permutation(V)[: n + 1].tolist() if V > 4096 else rng.choice(V, size=min(V, n + 1), replace=False).tolist()
    toks, fresh = perm[:n], perm[n] if len(perm) > n else None
    if edge and n >= 4:  # tokens 0 and V-1: first as history, last as a bias-only entry
        for want, at in ((0, 0), (V - 1, n - 1)):
            if want in toks:
                toks[toks.index(want)], toks[at] = toks[at], want
            elif want != fresh:
                toks[at] = want
    n_bias_only = min(n // 4, 40) if n >= 4 else 0
    hist, bias_only = toks[: n - n_bias_only], toks[n - n_bias_only:]
    n_prompt = (len(hist) + 1) // 2
    prompt_set, out_set = hist[:n_prompt], hist[n_prompt:]
    prompt = [prompt_set[i] for i in rng.integers(0, len(prompt_set), size=len(prompt_set) + 5)] + prompt_set \
        if prompt_set else []
    outputs = list(out_set)
    pool = out_set + prompt_set[: max(1, len(prompt_set) // 3)]  # tokens of the prompt generated again
    if pool and out_set:
        outputs += [pool[i] for i in rng.integers(0, len(pool), size=len(pool) // 2 + 3)]
    rng.shuffle(outputs)
    bias = {t: float(np.float32(rng.uniform(-5, 5))) for t in bias_only}
    for t in hist[:: max(1, len(hist) // 7)][:8]:  # bias on seen tokens too
        bias[t] = float(np.float32(rng.uniform(-5, 5)))
    rep, pres, freq = par
    sp = SamplingParams(repetition_penalty=rep, presence_penalty=pres, frequency_penalty=freq, logit_bias=bias)
    st = SeqProcState(prompt, bias)
    for t in outputs:
        st.add_output(t)
    assert st.n == n, (st.n, n)
    if oob:  # an entry past the vocabulary: the kernel must skip it, the oracle never sees it
        st.add_output(V + 5)
    pend_tok = None
    if pending == "hist" and hist:
        pend_tok = hist[int(rng.integers(0, len(hist)))]
    elif pending == "bias" and bias_only:
        pend_tok = bias_only[0]
    elif pending != "absent" and fresh is not None:
        pend_tok = fresh
    if pend_tok is not None:
        outputs = outputs + [pend_tok]
    return Row(prompt, outputs, sp, st, pend_tok)


@dataclass
class Case:
    logits: torch.Tensor     # [S, V] fp32 on the CPU, unprocessed
    expected: torch.Tensor   # [S, V] dense oracle
    rows: list               # Row or None (a plain row: stays bit-identical)
    pm: ProcMeta
    prev: torch.Tensor       # int32 [S + 3] previous sampler output (CPU)
    entries: int


def build_case(seed: int, V: int, specs: list, device="cpu", pm: ProcMeta | None = None, k: int = 0,
               bucket: int | None = None) -> Case:
    """``specs``: one (n_entries, pending, params index, oob) per row, or None for a plain row.
    ``bucket`` > len(specs) pads the step with empty rows, as the runner does."""
    rng = np.random.default_rng(seed)
    ns = len(specs)
    S = bucket or ns
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(S, V, generator=g) * 3.0
    logits[:, 7 % V] = 0.0  # a logit that is neither positive nor negative
    rows = [None if sp is None else make_row(rng, V, sp[0], sp[1], PARAMS[sp[2]], sp[3]) for sp in specs]
    if pm is None:
        pm = ProcMeta(S, V, 4096, device)
    prev = torch.full((S + 3,), -7, dtype=torch.int32)  # slots nobody points at hold garbage
    packed = []
    for s, r in enumerate(rows):
        if r is None:
            packed.append(None)
            continue
        pend = 0
        if r.pend_tok is not None:
            slot = (s * 5 + 1) % (S + 3)  # some slot of the previous step, not the row's own index
            while int(prev[slot]) != -7:
                slot = (slot + 1) % (S + 3)
            prev[slot] = r.pend_tok
            pend = -(slot + 1)
        packed.append((r.state, r.params, pend))
    n = pm.fill(k, packed, S)
    pm.upload(k)
    expected = logits.clone()
    for s, r in enumerate(rows):
        if r is not None:
            expected[s] = ref.process_logits_ref(logits[s], r.prompt, r.outputs, r.params)
    return Case(logits, expected, rows, pm, prev, n)
