"""Shaping of per-token log-probabilities between the engine and the chat API.

Three forms:

* engine: ``Sequence.logprobs``, one ``(token_id, logprob, [(id, logprob), ...])`` per output token;
* backend result: ``result["logprobs"] = [{"token_id", "logprob", "top": [[id, logprob], ...]}, ...]``
  (:func:`result_entries`); whoever owns the tokenizer adds ``"token"`` / ``"bytes"`` to each entry and
  ``"top_tokens": [[token, bytes], ...]`` beside ``top`` (:func:`annotate`): the API process for an
  in-process engine, the engine core for ``engine_process``, the worker for a remote gateway;
* response: ``choices[0].logprobs = {"content": [...]}`` in the OpenAI shape (:func:`content`).

JSON has no infinity: a ``-inf`` log-probability is written as ``-9999.0``.
"""
from __future__ import annotations

import math

NEG_INF_JSON = -9999.0


def _num(v: float) -> float:
    return float(v) if math.isfinite(v) else NEG_INF_JSON


def token_ids(entries) -> set:
    """Every token id the engine-form entries name (chosen tokens and alternatives)."""
    ids = set()
    for e in entries:
        if e is not None:
            ids.add(e[0])
            ids.update(t for t, _ in e[2])
    return ids


def result_entries(entries) -> list:
    """Engine form -> backend-result form (an entry the engine could not fill becomes an empty one)."""
    out = []
    for e in entries:
        if e is None:
            out.append({"token_id": -1, "logprob": NEG_INF_JSON, "top": []})
        else:
            out.append({"token_id": int(e[0]), "logprob": _num(e[1]), "top": [[int(t), _num(v)] for t, v in e[2]]})
    return out


def _tok(b: bytes) -> list:
    return [b.decode("utf-8", errors="replace"), list(b)]


def annotate(entries: list, decode) -> list:
    """Add token strings and bytes to backend-result entries, in place (entries that carry them are
    left alone). ``decode(token_id) -> bytes``."""
    for e in entries:
        if "token" in e:
            continue
        e["token"], e["bytes"] = _tok(decode(e["token_id"]) if e["token_id"] >= 0 else b"")
        e["top_tokens"] = [_tok(decode(t)) for t, _ in e["top"]]
    return entries


def annotate_result(result: dict, backend) -> dict:
    """Annotate a backend result's logprobs with the tokenizer of the backend's in-process engine, if
    it has one and the entries are still bare (results of workers and of an engine core process arrive
    annotated)."""
    entries = result.get("logprobs") if isinstance(result, dict) else None
    if not entries or "token" in entries[0]:
        return result
    tok = getattr(getattr(backend, "engine", None), "tokenizer", None)
    if tok is not None:
        annotate(entries, lambda t: tok.decode_bytes([t]))
    return result


def content(entries: list) -> list:
    """Annotated backend-result entries -> the ``content`` list of ``choices[0].logprobs``."""
    out = []
    for e in entries:
        tops = e.get("top_tokens") or [["", []]] * len(e["top"])
        out.append({"token": e.get("token", ""), "logprob": e["logprob"], "bytes": e.get("bytes", []),
                    "top_logprobs": [{"token": s, "logprob": v, "bytes": b}
                                     for (_, v), (s, b) in zip(e["top"], tops)]})
    return out
