"""Inputs and references for the tests at byte offsets past 2^31 and 2^32 (tests/test_far_*_gpu.py).

No reference reads a multi-GB buffer back. ``fill_by_position`` gives element ``e`` of a device tensor a value
that is a pure function of its 64-bit index, and ``expected`` evaluates the same function in numpy on ``uint64``
indices, so the expected content of any row or span is "this formula at these indices", pushed through the
independent references of tests/kernel_refs.py, tests/augment_refs.py and tests/reduction_refs.py.

A 32-bit wrap in a kernel's address arithmetic stays inside the allocation and delivers the elements 2^31 or
2^32 bytes (or elements) in front of the right ones. ``assert_no_alias`` checks, on the CPU and before the
launch, that those elements differ from the right ones under the formula, so such a wrap cannot pass unseen.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

BIG = (1 << 32) + (1 << 20)  # bytes of the sources that cross the 2^32 mark
MARKS = (1 << 31, 1 << 32, 1 << 33)  # byte offsets and element indices where 32-bit arithmetic breaks
FILL_CHUNK = 1 << 27  # elements per fill step
COMPARE_ROWS = 1 << 20  # rows per slice when a multi-GB output is compared

_M1, _M2 = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93
_BITS = {torch.uint8: 8, torch.int16: 16, torch.int32: 32}
_NP = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.float32: np.float32,
       torch.float16: np.float16}


def _signed(v: int) -> int:
    return v - (1 << 64) if v >= 1 << 63 else v


def _hash_torch(e: torch.Tensor) -> torch.Tensor:
    """Wrapping int64 multiply-shift hash; the masked shift makes the arithmetic shift a logical one."""
    x = e * _signed(_M1)
    x = x ^ ((x >> 32) & 0xFFFFFFFF)
    return x * _signed(_M2)


def _hash_np(e: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = e.astype(np.uint64) * np.uint64(_M1)
        x = x ^ (x >> np.uint64(32))
        return x * np.uint64(_M2)


def _top_torch(x: torch.Tensor, bits: int) -> torch.Tensor:
    return (x >> (64 - bits)) & ((1 << bits) - 1)


def _normal_from_bytes(s):
    """Four hash bytes summed (mean 510, variance 4 * (256^2 - 1) / 12): N(3, 1)-like, formed in float64."""
    return 3.0 + (s - 510.0) / 147.80054127  # sqrt(21845)


def _values_torch(e: torch.Tensor, dtype, kind) -> torch.Tensor:
    x = _hash_torch(e)
    if dtype in _BITS:
        bits = _BITS[dtype]
        v = _top_torch(x, bits)
        if dtype != torch.uint8:  # the same bits as a signed value, so that the narrowing cast is exact
            v = v - ((v >> (bits - 1)) << bits)
        return v.to(dtype)
    if kind == "ints":
        return _top_torch(x, 8).to(dtype)
    if kind == "normal":
        s = sum((x >> sh) & 0xFF for sh in (32, 40, 48, 56))
        return _normal_from_bytes(s.double()).to(dtype)
    raise ValueError(f"no fill for {dtype} / {kind}")


def expected(idx, dtype, kind=None) -> np.ndarray:
    """The values ``fill_by_position`` gives the elements ``idx`` (any shape, 64-bit indices), as numpy."""
    x = _hash_np(np.asarray(idx))
    if dtype in _BITS:
        bits = _BITS[dtype]
        v = x >> np.uint64(64 - bits)
        return v.astype({8: np.uint8, 16: np.uint16, 32: np.uint32}[bits]).view(_NP[dtype])
    if kind == "ints":
        return (x >> np.uint64(56)).astype(_NP[dtype])
    if kind == "normal":
        s = sum(((x >> np.uint64(sh)) & np.uint64(0xFF)).astype(np.float64) for sh in (32, 40, 48, 56))
        return _normal_from_bytes(s).astype(_NP[dtype])
    raise ValueError(f"no fill for {dtype} / {kind}")


def fill_by_position(t: torch.Tensor, kind=None) -> torch.Tensor:
    """Element ``e`` of the contiguous tensor ``t`` (in memory order) := f(e), in chunks of 2^27 elements.
    Integer dtypes get the full range of the dtype; float dtypes integers in [0, 255] (``kind="ints"``, exact
    under every conversion) or N(3, 1)-like values (``kind="normal"``)."""
    assert t.is_contiguous()
    flat = t.view(-1)
    for c0 in range(0, flat.numel(), FILL_CHUNK):
        c1 = min(c0 + FILL_CHUNK, flat.numel())
        flat[c0:c1] = _values_torch(torch.arange(c0, c1, dtype=torch.int64, device=t.device), t.dtype, kind)
    return t


def fill_value(t: torch.Tensor, value) -> torch.Tensor:
    """A constant fill in chunks (the sentinel of scatter destinations)."""
    flat = t.view(-1)
    for c0 in range(0, flat.numel(), FILL_CHUNK):
        flat[c0:c0 + FILL_CHUNK] = value
    return t


def expected_rows(rows, row_elems: int, dtype, kind=None) -> torch.Tensor:
    """CPU tensor [len(rows), row_elems]: what rows ``rows`` of a filled [n, row_elems] tensor hold."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    idx = rows * np.uint64(row_elems) + np.arange(row_elems, dtype=np.uint64)
    return torch.from_numpy(expected(idx, dtype, kind))


def expected_span(start: int, count: int, dtype, kind=None) -> torch.Tensor:
    return torch.from_numpy(expected(np.uint64(start) + np.arange(count, dtype=np.uint64), dtype, kind))


# ----------------------------------------------------------------------- marks
def _hashed(k: int, n: int) -> int:
    return int(_hash_np(np.array([k + 1], dtype=np.uint64))[0] % np.uint64(n))


def mark_rows(row_bytes: int, n_src: int, n_hashed: int = 3) -> list:
    """Rows of an [n_src, row_bytes] byte table where address arithmetic breaks: row 0, the rows just below, at
    and just above each byte mark the table reaches, row n_src - 1, and a few hash-chosen rows. Sorted, unique."""
    rows = {0, n_src - 1}
    for m in MARKS:
        r = m // row_bytes  # the row that holds byte offset m (starts at it when row_bytes divides m)
        rows.update(x for x in (r - 1, r, r + 1) if 0 <= x < n_src)
    rows.update(_hashed(k, n_src) for k in range(n_hashed))
    return sorted(rows)


def straddle_base(row_bytes: int, n_rows: int, mark: int = 1 << 32) -> int:
    """First row of ``n_rows`` consecutive rows with the byte offset ``mark`` in their middle."""
    return mark // row_bytes - n_rows // 2


def assert_no_alias(starts, count: int, dtype, kind=None, elem_bytes: int = 1) -> None:
    """The alias condition: for every span of ``count`` elements that starts at element ``x`` in ``starts``, the
    spans that start 2^31 and 2^32 bytes, and 2^31 and 2^32 elements, in front of it (where they exist) hold
    other values under the fill formula. A condition on the inputs, checked before the launch."""
    shifts = sorted({m // elem_bytes for m in MARKS[:2]} | set(MARKS[:2]))
    for x in starts:
        own = expected_span(int(x), count, dtype, kind)
        for s in shifts:
            if x - s >= 0:
                other = expected_span(int(x) - s, count, dtype, kind)
                assert not torch.equal(own, other), f"span at {x} equals the span {s} elements before it"


def need_hbm(nbytes: int) -> None:
    """Skip (with the figures) unless 1.5 x ``nbytes`` of device memory are free."""
    free = torch.cuda.mem_get_info()[0]
    if free < 1.5 * nbytes:
        pytest.skip(f"needs {1.5 * nbytes / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")
