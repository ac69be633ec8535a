"""A weighted mixture of the parts of one corpus, by document order ("code twice, web once, a quarter of the forum
dump": Megatron's blended dataset, the ``repeat`` / ``proportion`` of MosaicML Streaming).

``TokenMix(bounds, repeat)`` cuts the corpus's documents into ``P <= 16`` contiguous, non-empty parts
``[bounds[p], bounds[p + 1])`` and says how many times each appears per epoch. With ``n_p`` the documents of part
``p``::

    full_p = floor(repeat[p])                                whole passes over the part
    k_p    = floor((repeat[p] - full_p) * n_p + 0.5)         extra documents
    c_p    = full_p * n_p + k_p                              the part's entries in an epoch's order
    N'     = sum(c_p) >= 1                                   the order's length (``n_order``)

An epoch's order (``ops.ref_mix_order``, the definition; ``ops.token_mix_order``, the kernel) is a permutation of
those ``N'`` entries, and ``ResidentTokenStreamLoader(mix=...)`` cuts its rows from ``concat(document order_e[i])``.

The ``k_p`` extra documents of a part are the first ``k_p`` of one fixed permutation of the part
(``FeistelPermutation(n_p, part_seed_for(seed, p), 0)``): **the same documents in every epoch**, on purpose. The
epoch's token count is then one constant the host knows at construction, so rows per epoch, batches per epoch, the
row permutation's domain and the checkpoint cursor stay fixed, which the prefetching loader and ``shuffle_rows``
rely on. Resampling the subset every epoch is not offered.
"""

from __future__ import annotations

import math

import numpy as np

from .permutation import FeistelPermutation, part_seed_for

MAX_PARTS = 16


class TokenMix:
    def __init__(self, bounds, repeat):
        """``bounds``: ``P + 1`` strictly increasing document indices from 0 to the corpus's document count;
        ``repeat``: ``P`` finite numbers >= 0."""
        try:
            self.bounds = tuple(int(b) for b in bounds)
            self.repeat = tuple(float(r) for r in repeat)
            exact = all(int(b) == b for b in bounds)
        except (TypeError, ValueError) as e:
            raise ValueError(f"bounds must be integers and repeat numbers: {e}") from None
        if not exact:
            raise ValueError("bounds must be integers")
        P = len(self.repeat)
        if not 1 <= P <= MAX_PARTS:
            raise ValueError(f"a mix has 1 to {MAX_PARTS} parts, not {P}")
        if len(self.bounds) != P + 1:
            raise ValueError(f"{P} parts need {P + 1} bounds, not {len(self.bounds)}")
        if self.bounds[0] != 0 or any(b1 <= b0 for b0, b1 in zip(self.bounds, self.bounds[1:])):
            raise ValueError("bounds must start at 0 and increase strictly (parts are not empty)")
        if any(not math.isfinite(r) or r < 0 for r in self.repeat):
            raise ValueError("every repeat must be finite and >= 0")
        self.n_docs = tuple(b1 - b0 for b0, b1 in zip(self.bounds, self.bounds[1:]))
        self.full = tuple(int(math.floor(r)) for r in self.repeat)
        self.extra = tuple(int(math.floor((r - f) * n + 0.5)) for r, f, n in zip(self.repeat, self.full, self.n_docs))
        self.counts = tuple(f * n + k for f, n, k in zip(self.full, self.n_docs, self.extra))
        self.cbase = tuple(int(c) for c in np.concatenate([[0], np.cumsum(self.counts, dtype=np.int64)]))
        self.n_order = self.cbase[-1]
        self.max_copies = tuple(f + (1 if k else 0) for f, k in zip(self.full, self.extra))
        if self.n_order < 1:
            raise ValueError("the mix selects no document at all")
        if self.n_order >= 1 << 62:
            raise ValueError("the mix's order does not fit int64 positions")

    @classmethod
    def from_weights(cls, bounds, part_tokens, weights, epoch_tokens=None) -> "TokenMix":
        """The mix in which part ``p`` makes the share ``weights[p] / sum(weights)`` of an epoch of ``epoch_tokens``
        tokens (default: ``sum(part_tokens)``, the corpus's size): ``repeat[p] = w_p / sum(w) * epoch_tokens /
        part_tokens[p]``. The share is met up to the rounding of ``k_p`` and the lengths of the extra documents."""
        toks = [int(t) for t in part_tokens]
        w = [float(x) for x in weights]
        if len(toks) != len(w):
            raise ValueError("part_tokens and weights must have one entry per part")
        if any(not math.isfinite(x) or x < 0 for x in w) or not sum(w) > 0:
            raise ValueError("weights must be finite, >= 0 and not all zero")
        if any(t < 0 for t in toks):
            raise ValueError("part_tokens must be >= 0")
        total = float(sum(toks) if epoch_tokens is None else epoch_tokens)
        if not math.isfinite(total) or total <= 0:
            raise ValueError("epoch_tokens must be positive")
        sw = sum(w)
        repeat = []
        for p, (t, x) in enumerate(zip(toks, w)):
            if x > 0 and t == 0:
                raise ValueError(f"part {p} has weight {x} and no tokens")
            repeat.append(x * total / (sw * t) if x > 0 else 0.0)  # one rounding: exact where the ratio is
        return cls(bounds, repeat)

    @property
    def parts(self) -> int:
        return len(self.repeat)

    @property
    def n_documents(self) -> int:
        return self.bounds[-1]

    def inner_perm(self, seed: int, part: int) -> FeistelPermutation:
        """``sigma_p``: the fixed permutation of part ``part`` whose first ``k_p`` values are its extra documents."""
        return FeistelPermutation(self.n_docs[part], part_seed_for(seed, part), 0)

    def extra_documents(self, seed: int, part: int, shuffle: bool = True) -> np.ndarray:
        """Corpus ids of the ``k_p`` documents of ``part`` that appear ``full_p + 1`` times, the same every epoch."""
        r = np.arange(self.extra[part], dtype=np.int64)
        if shuffle and r.size:
            r = np.asarray(self.inner_perm(seed, part)(r), dtype=np.int64)
        return self.bounds[part] + r

    def epoch_tokens(self, lengths, seed: int, shuffle: bool = True) -> int:
        """Tokens of one epoch (any epoch) over documents of ``lengths``: the whole passes from the parts' totals,
        the extras from their documents' lengths."""
        lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if lens.size != self.n_documents:
            raise ValueError(f"the mix covers {self.n_documents} documents, the corpus has {lens.size}")
        total = 0
        for p in range(self.parts):
            total += self.full[p] * int(lens[self.bounds[p]:self.bounds[p + 1]].sum())
            total += int(lens[self.extra_documents(seed, p, shuffle)].sum())
        return total

    def document_copies(self) -> np.ndarray:
        """``max_copies`` of every document's part, int64 [n_documents]: the most a document appears in an epoch."""
        return np.repeat(np.asarray(self.max_copies, dtype=np.int64), self.n_docs)

    def device_args(self, seed: int, shuffle: bool = True) -> dict:
        """The part table of the ``token_mix_order`` launcher (the epoch's outer selector is the caller's)."""
        inner = [self.inner_perm(seed, p) for p in range(self.parts)] if shuffle else []
        return dict(cbase=list(self.cbase), doc_lo=list(self.bounds[:-1]), n_docs=list(self.n_docs),
                    full_span=[f * n for f, n in zip(self.full, self.n_docs)], inner_shuffle=bool(shuffle),
                    inner_keys=[s.keys for s in inner], inner_half_bits=[s.half_bits for s in inner])

    def state(self) -> dict:
        """What a checkpoint keeps of the mix: two mixes with the same bounds and counts give the same orders."""
        return {"bounds": list(self.bounds), "counts": list(self.counts)}

    def __repr__(self) -> str:
        return f"TokenMix(bounds={list(self.bounds)}, repeat={list(self.repeat)})"
