"""Request/response models (OpenAI-shaped Chat Completions subset)."""
from __future__ import annotations

from typing import Optional

from pydantic import BaseModel, Field


class ChatMessage(BaseModel):
    role: str
    content: str


class ChatCompletionRequest(BaseModel):
    model: str
    messages: list[ChatMessage]
    temperature: float = 0.7
    top_p: float = 0.9
    max_tokens: int = 256
    stream: bool = False
    # optional sampling controls: left out of the request body unless given
    presence_penalty: Optional[float] = None
    frequency_penalty: Optional[float] = None
    repetition_penalty: Optional[float] = None
    logit_bias: Optional[dict[str, float]] = None
    seed: Optional[int] = None
    top_k: Optional[int] = None
    # per-token log-probabilities (non-streaming): logprobs = True, top_logprobs = 0..20 alternatives
    logprobs: Optional[bool] = None
    top_logprobs: Optional[int] = None


class EmbeddingRequest(BaseModel):
    model: str
    input: str


class Usage(BaseModel):
    prompt_tokens: int = 0
    completion_tokens: int = 0
    total_tokens: int = 0


class ResponseMessage(BaseModel):
    role: str
    content: str


class TopLogprob(BaseModel):
    token: str
    logprob: float
    bytes: Optional[list[int]] = None


class TokenLogprob(BaseModel):
    token: str
    logprob: float  # -9999.0 stands for -inf (a token of probability zero)
    bytes: Optional[list[int]] = None
    top_logprobs: list[TopLogprob] = Field(default_factory=list)


class ChoiceLogprobs(BaseModel):
    content: Optional[list[TokenLogprob]] = None


class Choice(BaseModel):
    index: int
    message: ResponseMessage
    finish_reason: Optional[str] = None
    logprobs: Optional[ChoiceLogprobs] = None


class ChatCompletion(BaseModel):
    id: str
    object: str = "chat.completion"
    created: int
    model: str
    choices: list[Choice]
    usage: Usage = Field(default_factory=Usage)


class ChatCompletionDelta(BaseModel):
    role: Optional[str] = None
    content: Optional[str] = None


class ChatCompletionChunkChoice(BaseModel):
    index: int
    delta: ChatCompletionDelta
    finish_reason: Optional[str] = None


class ChatCompletionChunk(BaseModel):
    id: str
    object: str = "chat.completion.chunk"
    created: int
    model: str
    choices: list[ChatCompletionChunkChoice]


class EmbeddingData(BaseModel):
    object: str = "embedding"
    embedding: list[float]
    index: int


class EmbeddingResponse(BaseModel):
    object: str = "list"
    data: list[EmbeddingData]
    model: str
    usage: Usage = Field(default_factory=Usage)


class HealthResponse(BaseModel):
    status: str
    version: str


class RateLimitInfo(BaseModel):
    limit: Optional[int] = None
    remaining: Optional[int] = None
    reset: Optional[float] = None
    retry_after: Optional[float] = None
