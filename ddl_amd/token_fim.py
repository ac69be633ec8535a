"""Fill-in-the-middle (FIM) rearrangement of token rows, the transformation code models are pre-trained with
(StarCoder, Code Llama, DeepSeek-Coder, the bigcode fork of Megatron's GPT dataset): a share of the document pieces
in a row is rewritten as ``<PRE> prefix <SUF> suffix <MID> middle`` (PSM) or ``<PRE> <SUF> suffix <MID> prefix
middle`` (SPM), the row's length unchanged.

``TokenFIM(rate, prefix_id=, middle_id=, suffix_id=, spm_rate=0.5, eod_id=None, min_len=8)`` is the specification;
``ops.ref_fim_tokens`` is the definition, ``ops.fim_tokens`` the kernel, and ``fim=`` of the token stream loaders
applies it to every batch on the device. Everything is integer arithmetic. With ``rate_q = round(rate * 2**24)``,
``spm_q`` likewise, and per epoch one 64-bit ``ekey = mix64(fim_seed_for(seed) + (epoch + 1) * 0x9E3779B97F4A7C15)``,
a segment -- a maximal run of one document in one row -- of tokens ``t[0 .. L)`` with key ``k``::

    u_c  = mix64(ekey ^ mix64(4 * k + c)),  c = 0 .. 3        (k as uint64, sums modulo 2**64)
    tail = 1 if eod_id is given and t[L - 1] == eod_id else 0;   M = L - tail;   K = M - 3
    rearranged iff M >= min_len and (u_0 >> 40) < rate_q;        SPM iff (u_1 >> 40) < spm_q, else PSM
    x = ((u_2 >> 32) * (K + 1)) >> 32,  y likewise of u_3;       a = min(x, y),  b = max(x, y)
    prefix = t[0 .. a),  middle = t[a .. b),  suffix = t[b .. K)
    PSM:  [prefix_id] prefix [suffix_id] suffix [middle_id] middle     (+ t[L - 1] if tail)
    SPM:  [prefix_id] [suffix_id] suffix [middle_id] prefix middle     (+ t[L - 1] if tail)

The three body tokens ``t[K .. M)`` are dropped to make room for the sentinels (the truncate mode of the bigcode
implementation, which shortens the suffix), so the segment keeps its ``L`` positions; a piece of a document cut by a
row boundary is a segment like any other. Padding, ``attention_mask``, ``position_ids``, ``segment_ids`` and
``cu_seqlens`` are unchanged, and labels are ``ref_token_labels`` of the rearranged ids.

In the loaders a segment's key is the corpus element of its first token, so with the epoch its rearrangement does
not depend on the world size, the rank, ``shuffle_rows``, the batch its row lands in or where the tokens are read
from. One limit follows: with a ``TokenMix``, two copies of a document in one epoch get the same cuts where their
pieces start at the same token.
"""

from __future__ import annotations

import math

from .permutation import _MASK64, _mix64_int, fim_seed_for

_Q = 1 << 24


def _quantise(name: str, x) -> int:
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number in [0, 1], got {x!r}") from None
    if not math.isfinite(v) or not 0.0 <= v <= 1.0:
        raise ValueError(f"{name} must lie in [0, 1], got {x!r}")
    return int(round(v * _Q))


def _int32(name: str, x) -> int:
    try:
        v = int(x)
        exact = v == x
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an integer, got {x!r}") from None
    if not exact or isinstance(x, bool) or not -(1 << 31) <= v < (1 << 31):
        raise ValueError(f"{name} must be an int32 value, got {x!r}")
    return v


class TokenFIM:
    def __init__(self, rate, *, prefix_id, middle_id, suffix_id, spm_rate=0.5, eod_id=None, min_len=8):
        """``rate``: the share of eligible segments rearranged; ``spm_rate``: the SPM share among them (both in
        [0, 1], quantised to 24 bits once); the three sentinel ids and ``eod_id`` (None: no segment has an EOD
        tail) are int32 values; ``min_len`` >= 4: the shortest body, without its EOD, that is rearranged."""
        self.rate_q = _quantise("rate", rate)
        self.spm_q = _quantise("spm_rate", spm_rate)
        self.prefix_id = _int32("prefix_id", prefix_id)
        self.middle_id = _int32("middle_id", middle_id)
        self.suffix_id = _int32("suffix_id", suffix_id)
        self.eod_id = None if eod_id is None else _int32("eod_id", eod_id)
        self.min_len = _int32("min_len", min_len)
        if self.min_len < 4:
            raise ValueError(f"min_len must be >= 4 (three sentinels and a token), got {min_len!r}")

    @property
    def rate(self) -> float:
        return self.rate_q / _Q

    @property
    def spm_rate(self) -> float:
        return self.spm_q / _Q

    def epoch_key(self, seed: int, epoch: int) -> int:
        """``ekey`` of (seed, epoch): the only random state the kernel gets."""
        return _mix64_int((fim_seed_for(seed) + (int(epoch) + 1) * 0x9E3779B97F4A7C15) & _MASK64)

    def device_args(self, seed: int, epoch: int) -> dict:
        """The specification as the ``token_fim`` launcher takes it."""
        return dict(ekey=self.epoch_key(seed, epoch), rate_q=self.rate_q, spm_q=self.spm_q, prefix_id=self.prefix_id,
                    middle_id=self.middle_id, suffix_id=self.suffix_id, has_eod=self.eod_id is not None,
                    eod_id=0 if self.eod_id is None else self.eod_id, min_len=self.min_len)

    def state(self) -> dict:
        """What a checkpoint keeps: two specifications with the same state rearrange alike."""
        return {"rate_q": self.rate_q, "spm_q": self.spm_q, "prefix_id": self.prefix_id, "middle_id": self.middle_id,
                "suffix_id": self.suffix_id, "eod_id": self.eod_id, "min_len": self.min_len}

    def __repr__(self) -> str:
        return (f"TokenFIM({self.rate!r}, prefix_id={self.prefix_id}, middle_id={self.middle_id}, "
                f"suffix_id={self.suffix_id}, spm_rate={self.spm_rate!r}, eod_id={self.eod_id}, "
                f"min_len={self.min_len})")
