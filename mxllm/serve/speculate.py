"""Drafts for speculative decoding without a second model: prompt lookup.

The request's own text proposes its continuation.  For the last ``g`` tokens of prompt + output
(``g`` from ``MAX_NGRAM`` = 3 down to 1) the most recent EARLIER occurrence of that n-gram is looked up
and the tokens that followed it are proposed, at most ``k``.  The longest n-gram that has an earlier
occurrence wins; without any there is no draft.  Summaries, code edits, retrieval answers and any
output that repeats its prompt or itself draft well; free text mostly does not, and then the step is
the plain one.

The engine (mxllm/serve/engine.py ``Engine(speculate=K)``) verifies a draft in one step: the last
token and the drafts are ``1 + len(draft)`` rows of the sequence, the sampler draws on every row, and
draft ``j + 1`` is accepted iff row ``j`` drew it (``mxllm.ops.decode.spec_accept``) -- the proposal
is deterministic, so this is exact speculative sampling and the token stream is the plain engine's.

A drafter is any callable ``(tokens: list[int], k: int) -> list[int]``; ``prompt_lookup`` is the
stateless one.  ``NgramIndex`` is its incremental form, one per request: a dict from n-gram to the
last position it ended at, updated per appended token, so the host cost of a step does not grow
with the context.
"""
from __future__ import annotations

MAX_NGRAM = 3


def prompt_lookup(tokens: list[int], k: int) -> list[int]:
    """The draft for ``tokens`` by a from-scratch search (see the module docstring): at most ``k``
    tokens, [] without a match."""
    n = len(tokens)
    if k <= 0:
        return []
    for g in range(min(MAX_NGRAM, n - 1), 0, -1):
        tail = tokens[n - g:]
        for i in range(n - 2, g - 2, -1):  # i: where the earlier occurrence ends (it has a follower)
            if tokens[i - g + 1:i + 1] == tail:
                return list(tokens[i + 1:i + 1 + k])
    return []


class NgramIndex:
    """``prompt_lookup`` kept incrementally.  ``last[ngram]`` is the last position < len - 1 at which
    the n-gram ends: an n-gram ending at position p is entered when token p + 1 arrives, so the
    current tail never finds itself and every hit has a follower."""

    def __init__(self, tokens=()):
        self.tokens: list[int] = []
        self.last: dict[tuple, int] = {}
        self.extend(tokens)

    def __len__(self) -> int:
        return len(self.tokens)

    def append(self, tok: int) -> None:
        p = len(self.tokens)  # the position of tok; the n-grams ending at p - 1 now have a follower
        for g in range(1, min(MAX_NGRAM, p) + 1):
            self.last[tuple(self.tokens[p - g:p])] = p - 1
        self.tokens.append(int(tok))

    def extend(self, toks) -> None:
        for t in toks:
            self.append(t)

    def propose(self, k: int) -> list[int]:
        n = len(self.tokens)
        if k <= 0:
            return []
        for g in range(min(MAX_NGRAM, n - 1), 0, -1):
            i = self.last.get(tuple(self.tokens[n - g:]))
            if i is not None:
                return self.tokens[i + 1:i + 1 + k]
        return []

    def sync(self, tokens: list[int]) -> None:
        """Bring the index up to ``tokens``, which extends what it holds (a request's prompt +
        output only grows)."""
        self.extend(tokens[len(self.tokens):])
