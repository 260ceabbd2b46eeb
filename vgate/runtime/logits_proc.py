"""Host state of the logits processors (penalties, logit_bias) and their per-step device buffer.

A sequence whose ``params.has_processors`` is true carries a :class:`SeqProcState`: ONE 16-byte
entry per unique token of its prompt, its output and its ``logit_bias`` —
``{tok:int32, cnt:int32, bias:float32, pad}``, bit 31 of ``cnt`` = "occurs in the prompt", the low
bits = occurrences in the output. It depends on ``prompt_ids`` and ``output_ids`` only, so prefix-cache
hits, chunked prefill and recompute preemption need nothing special; the engine bumps a count in
O(1) whenever an output token becomes known (``LLMEngine._process``).

:class:`ProcMeta` is the step buffer the logits kernel reads (csrc/kernels/logits_proc.hip): a header
``row_off[S+1]``, ``pend[S]``, ``par[S] = {rep, inv_rep, pres, freq}`` and the rows' entries packed
back to back. Like :class:`StepMeta` it has two pinned host buffers (asynchronous scheduling fills
step t+1 while step t's copy may be queued) and one fixed-address device buffer that captured
graphs read; it is allocated on the first processor step and never regrown.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from vgate import ops

ENTRY = np.dtype([("tok", np.int32), ("cnt", np.int32), ("bias", np.float32), ("pad", np.int32)])
IN_PROMPT = np.int32(-(1 << 31))  # bit 31 of cnt
MAX_BIAS = 300  # logit_bias entries per request the step buffer is sized for


def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


def check_request(params, vocab_size: int, tp_size: int = 1) -> None:
    """Admission check of a request's processors (LLMEngine.add_request, and the engine-process
    client before the request crosses the pipe): ValueError for what the engine cannot serve."""
    if not params.has_processors:
        return
    if tp_size > 1:
        # the TP step ring ships StepMeta only: followers would sample unprocessed logits
        raise ValueError("penalties and logit_bias are not supported with tensor parallelism")
    bad = [t for t in params.logit_bias if t >= vocab_size]
    if bad:
        raise ValueError(f"logit_bias token id {bad[0]} is outside the vocabulary ({vocab_size})")
    if len(params.logit_bias) > MAX_BIAS:
        raise ValueError(f"logit_bias holds more than {MAX_BIAS} entries")


def check_logprobs(params, tp_size: int = 1) -> None:
    """Admission check of a logprobs request (same callers as :func:`check_request`)."""
    if getattr(params, "logprobs", None) is None:
        return
    if tp_size > 1:
        # the TP step ring ships StepMeta only: followers would not know which rows asked
        raise ValueError("logprobs are not supported with tensor parallelism")


class SeqProcState:
    """Unique-token entries of one sequence (prompt tokens, output tokens, biased tokens)."""

    def __init__(self, prompt_ids, logit_bias: dict | None = None):
        uniq = np.unique(np.asarray(prompt_ids, dtype=np.int64)) if len(prompt_ids) else np.zeros(0, np.int64)
        bias = logit_bias or {}
        in_prompt = set(uniq.tolist())
        extra = [int(t) for t in bias if int(t) not in in_prompt]
        n = len(uniq) + len(extra)
        self.arr = np.zeros(max(64, 2 * n), dtype=ENTRY)
        self.arr["tok"][: len(uniq)] = uniq
        self.arr["cnt"][: len(uniq)] = IN_PROMPT
        self.arr["tok"][len(uniq): n] = extra
        self.n = n
        self.index = {int(t): i for i, t in enumerate(self.arr["tok"][:n].tolist())}
        for t, b in bias.items():
            self.arr["bias"][self.index[int(t)]] = b

    def add_output(self, tok: int) -> None:
        """One more occurrence of ``tok`` in the output (appended, or a PENDING slot resolved)."""
        i = self.index.get(tok)
        if i is None:
            if self.n == len(self.arr):
                self.arr = np.concatenate([self.arr, np.zeros(len(self.arr), dtype=ENTRY)])
            i = self.index[tok] = self.n
            self.arr["tok"][i] = tok
            self.n += 1
        self.arr["cnt"][i] += 1

    def entries(self) -> np.ndarray:
        return self.arr[: self.n]


@dataclass
class ProcView:
    """Device views of one step's processor buffer (what ``ops.process_logits`` takes)."""
    S: int
    row_off: torch.Tensor   # int32 [S + 1]
    pend: torch.Tensor      # int32 [S]
    par: torch.Tensor       # fp32 [S, 4]
    entries: torch.Tensor   # int32 [capacity, 4]


def pack_params(sp) -> tuple:
    """{rep, inv_rep, pres, freq} as the kernel reads them: inv_rep = float32(1) / float32(rep)."""
    rep = np.float32(sp.repetition_penalty)
    return rep, np.float32(1.0) / rep, np.float32(sp.presence_penalty), np.float32(sp.frequency_penalty)


class ProcMeta:
    def __init__(self, max_seqs: int, vocab: int, max_model_len: int, device, pinned: bool = True):
        self.S = max_seqs
        self.device = torch.device(device)
        self.capacity = max_seqs * (min(vocab, max_model_len) + MAX_BIAS)
        off = 0
        self.layout = {}
        for name, dt, n in (("row_off", np.int32, self.S + 1), ("pend", np.int32, self.S),
                            ("par", np.float32, 4 * self.S), ("entries", np.int32, 4 * self.capacity)):
            off = _align(off)
            self.layout[name] = (off, dt, n)
            off += 4 * n
        self.nbytes = _align(off)
        self.header_bytes = self.layout["entries"][0]
        gpu = self.device.type == "cuda"
        self.hosts = [torch.zeros(self.nbytes, dtype=torch.uint8, pin_memory=pinned and gpu)
                      for _ in range(2 if gpu else 1)]
        self.dev = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device) if gpu else self.hosts[0]
        self._h = []
        for host in self.hosts:
            hnp = host.numpy()
            h = {name: hnp[o: o + 4 * n].view(dt) for name, (o, dt, n) in self.layout.items()}
            h["par"] = h["par"].reshape(self.S, 4)
            h["entries"] = hnp[self.header_bytes: self.header_bytes + 16 * self.capacity].view(ENTRY)
            self._h.append(h)
        tdt = {np.int32: torch.int32, np.float32: torch.float32}
        self.d = {name: self.dev[o: o + 4 * n].view(tdt[dt]) for name, (o, dt, n) in self.layout.items()}
        self.d["par"] = self.d["par"].view(self.S, 4)
        self.d["entries"] = self.d["entries"].view(self.capacity, 4)
        self.used = 0  # entries of the last fill

    def fill(self, k: int, rows, S: int) -> int:
        """Write host buffer ``k`` for a step of bucket ``S``: ``rows`` = one (state, params, pend) per
        batch item, or None for a row that gets an empty range (plain request, or a chunk that does
        not sample). Returns the number of entries packed (0 = not a processor step)."""
        h = self._h[k]
        ro, pd, par, ent = h["row_off"], h["pend"], h["par"], h["entries"]
        off = 0
        ro[0] = 0
        for s, row in enumerate(rows):
            if row is None:
                pd[s] = 0
            else:
                st, sp, pend = row
                n = st.n
                if off + n > self.capacity:
                    raise RuntimeError("logits-processor step buffer overflow")
                ent[off: off + n] = st.arr[:n]
                off += n
                par[s] = pack_params(sp)
                pd[s] = pend
            ro[s + 1] = off
        ns = len(rows)
        ro[ns + 1: S + 1] = off
        pd[ns:S] = 0
        self.used = off
        return off

    def fill_empty(self, k: int, S: int) -> None:
        """All-empty header (graph capture on padding metadata: the kernel's blocks exit at once)."""
        h = self._h[k]
        h["row_off"][: S + 1] = 0
        h["pend"][:S] = 0
        self.used = 0

    def upload(self, k: int) -> None:
        """Host buffer ``k`` -> device: the header and the used entries only (16-B pieces)."""
        if self.dev is self.hosts[k]:
            return
        ops.host_device_copy(self.dev, self.hosts[k], self.header_bytes + 16 * self.used)

    def view(self, S: int) -> ProcView:
        d = self.d
        return ProcView(S=S, row_off=d["row_off"][: S + 1], pend=d["pend"][:S], par=d["par"][:S],
                        entries=d["entries"])
