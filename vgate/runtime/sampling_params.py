"""Per-request sampling parameters for the native engine."""
from __future__ import annotations

import math
from dataclasses import dataclass, field


@dataclass
class SamplingParams:
    temperature: float = 0.7
    top_p: float = 0.9
    top_k: int = -1
    max_tokens: int = 256
    seed: int | None = None
    stop_token_ids: list[int] = field(default_factory=list)
    stop: list[str] = field(default_factory=list)
    ignore_eos: bool = False
    min_tokens: int = 0
    # logits processors (csrc/kernels/logits_proc.hip), applied to the raw logits before temperature:
    # repetition covers prompt + output tokens, presence / frequency the output tokens only
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: dict[int, float] = field(default_factory=dict)
    # per-token log-probabilities (csrc/kernels/logprobs.hip): None = off, k = 0..20 reports every
    # generated token's log-probability and the k most likely tokens with theirs, under the softmax at
    # temperature 1 of the logits as the sampler reads them (after the processors above)
    logprobs: int | None = None

    def __post_init__(self):
        if self.logprobs is not None:
            if isinstance(self.logprobs, bool) or not isinstance(self.logprobs, int) or not 0 <= self.logprobs <= 20:
                raise ValueError("logprobs must be an integer in 0..20")
        if self.temperature < 0:
            raise ValueError("temperature must be >= 0")
        if not (0.0 < self.top_p <= 1.0):
            raise ValueError("top_p must be in (0, 1]")
        if self.max_tokens < 1:
            raise ValueError("max_tokens must be >= 1")
        if self.top_k == 0:
            self.top_k = -1
        if not (math.isfinite(self.repetition_penalty) and self.repetition_penalty > 0):
            raise ValueError("repetition_penalty must be finite and > 0")
        if not (math.isfinite(self.presence_penalty) and math.isfinite(self.frequency_penalty)):
            raise ValueError("presence_penalty and frequency_penalty must be finite")
        if self.logit_bias:
            bias = {}
            for k, v in self.logit_bias.items():
                k, v = int(k), float(v)
                if k < 0:
                    raise ValueError("logit_bias keys must be token ids >= 0")
                if not math.isfinite(v):
                    raise ValueError("logit_bias values must be finite")
                bias[k] = v
            self.logit_bias = bias
        else:
            self.logit_bias = {}

    @property
    def greedy(self) -> bool:
        return self.temperature <= 1e-5

    @property
    def has_processors(self) -> bool:
        """Any logits processor differs from its default (the step then runs the logits kernel)."""
        return (self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0
                or bool(self.logit_bias))
