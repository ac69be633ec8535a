"""Independent float64 references, comparison rules and case tables for the row and collate kernels.

Nothing here calls a project op: the references are numpy / torch on the CPU, in float64, written from the
ops' documented meaning. ``tests/test_kernel_refs.py`` runs the tables through the ops on CPU tensors (the
project's ``ref_*`` paths), ``tests/test_kernels_matrix_gpu.py`` through the HIP kernels.

Rounding model of every converting op: the affine ``x * scale[ch] + bias[ch]`` is evaluated once in float32
(the kernels use one fused multiply-add with float32 ``scale`` / ``bias``), then cast to the output dtype with
round-to-nearest-even. The references evaluate it in float64 with the float32 values of ``scale`` / ``bias``,
round to float32 and cast with torch's CPU cast (RNE).

* Exact affines (``exact_affine``): every product and sum is exactly representable in float32, so no rounding
  happens before the final cast and outputs must be bit-identical (``assert_same``).
* Realistic affines (``realistic_affine``): float64-then-float32 rounds twice where the fused multiply-add rounds
  once; the two float32 values can differ by one float32 ulp, hence by at most one ulp of the output dtype
  after the final cast. ``assert_within_ulp(out, ref, 1)`` is for these cases only.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

from ddl_amd.permutation import FeistelPermutation

U8, F16, BF16, F32, I32, I64 = torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.int32, torch.int64

N_SRC = 13  # source rows of every gather / collate case; 5..9 of them are gathered
HOWS = ("identity", "index", "perm")
IN_DTYPES = (U8, F16, BF16, F32)
OUT_DTYPES = (BF16, F16, F32)
CAST_PAIRS = tuple((i, o) for i in IN_DTYPES for o in OUT_DTYPES if i != o)  # same dtype: the move path
AFFINE_PAIRS = CAST_PAIRS + ((F32, F32), (BF16, BF16), (F16, F16))
# around the chunked kernels' 2048-element threshold and their 8192 / 16384-element chunks
ROW_ELEMS = (1, 7, 2040, 2047, 2048, 2056, 8192, 8200, 16384, 16392, 24584)
AFFINE_CHANNELS = (1, 3, 4, 5, 16)
MISALIGNED_ROW_ELEMS = 8192

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def name(dtype) -> str:
    return str(dtype).replace("torch.", "")


# ------------------------------------------------------------------ addressing
class Rows:
    """Source rows of one case: ``rows`` (int64 CPU tensor) and the matching op keywords."""

    def __init__(self, rows, how, base=0, perm=None):
        self.rows = torch.as_tensor(np.ascontiguousarray(rows), dtype=torch.int64)
        self.how, self.base, self.perm = how, base, perm

    def __len__(self):
        return self.rows.numel()

    def kw(self, device="cpu") -> dict:
        if self.how == "index":
            return dict(index=self.rows.to(device))
        if self.how == "perm":
            return dict(perm=self.perm, base=self.base, n_rows=len(self))
        return dict(base=self.base, n_rows=len(self))


def rows_of(n_src: int, n_rows: int, how: str, seed: int = 0) -> Rows:
    """identity: rows base .. base + n_rows - 1 with base = 3; index: unsorted, with a repeat, touching the first
    and the last source row (for n_rows >= 3); perm: positions 2 .. of a host-evaluated FeistelPermutation."""
    if how == "identity":
        assert 3 + n_rows <= n_src
        return Rows(np.arange(3, 3 + n_rows), how, base=3)
    if how == "index":
        idx = np.random.default_rng(seed).integers(0, n_src, n_rows)
        if n_rows >= 3:
            idx[0], idx[1], idx[-1] = n_src - 1, 0, n_src - 1
        return Rows(idx, how)
    if how == "perm":
        p = FeistelPermutation(n_src, seed=seed + 1, epoch=seed % 3)
        assert 2 + n_rows <= n_src
        return Rows(p(np.arange(2, 2 + n_rows, dtype=np.int64)), how, base=2, perm=p)
    raise ValueError(how)


def n_gathered(seed: int) -> int:
    return 5 + seed % 5


# --------------------------------------------------------------------- sources
@functools.lru_cache(maxsize=64)
def _source(dtype, shape, kind, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    if dtype in (U8,):
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.int64)
        x.view(-1)[:2] = torch.tensor([0, 255])[: x.numel()]
        return x.to(U8)
    if dtype in (I32, I64):
        info = torch.iinfo(dtype)
        x = torch.randint(info.min // 2, info.max // 2, shape, generator=g, dtype=torch.int64) * 2 + 1
        return x.to(dtype)
    if kind == "ints":  # small integers: exact in every float dtype, and under an exact affine
        return torch.randint(-64, 64, shape, generator=g, dtype=torch.int64).to(dtype)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * 3).to(dtype)


def make_source(dtype, shape, kind="real", seed=0) -> torch.Tensor:
    """A fresh CPU tensor: uint8 pixels, odd integers of the full range (int32 / int64), small integers
    (``kind="ints"``) or N(0, 3) values rounded to ``dtype``."""
    return _source(dtype, tuple(shape), kind, seed).clone()


GUARD = 42  # fill of the elements around an offset view; checked to be untouched


def offset_buffer(shape, dtype, device, k: int = 1):
    """(buf, view): ``view = buf[k : k + numel].view(shape)`` of a fresh GUARD-filled allocation, contiguous and
    ``k`` elements off the allocation's alignment; ``k`` guard elements follow it too."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * k,), GUARD, dtype=dtype, device=device)
    return buf, buf[k:k + n].view(tuple(shape))


def offset_view(t: torch.Tensor, k: int = 1) -> torch.Tensor:
    """A contiguous copy of ``t`` (on its device) that starts ``k`` elements into a fresh allocation."""
    _, v = offset_buffer(t.shape, t.dtype, t.device, k)
    v.copy_(t)
    return v


def assert_guards(buf: torch.Tensor, k: int, what: str = "") -> None:
    g = torch.cat([buf[:k], buf[-k:]]).cpu()
    assert bool((g == GUARD).all()), f"{what}: elements outside the offset view were written: {g.tolist()}"


# --------------------------------------------------------------------- affines
def _f32(values):
    return [float(np.float32(v)) for v in values]


def exact_affine(channels: int):
    """scale 2^-(1 + c % 5), bias (c - 7) / 16: distinct per channel, and exact in float32 on uint8 pixels and
    on integers in [-64, 64)."""
    return [2.0 ** -(1 + c % 5) for c in range(channels)], [(c - 7) / 16 for c in range(channels)]


def realistic_affine(in_dtype):
    """ImageNet mean / std through ``norm_affine``, as the float32 values the kernels receive."""
    from ddl_amd.ops import norm_affine, pixel_max

    sc, bi = norm_affine(3, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], None, None, pixel_max(in_dtype))
    return _f32(sc), _f32(bi)


def plane_for(row_elems: int, channels: int) -> int:
    """``channels * plane == row_elems`` where that divides; otherwise the largest multiple of 8 below
    ``row_elems / channels`` (the row's tail wraps to channel 0 and the vector kernels stay reachable), or the
    plain quotient for rows too short for that."""
    if row_elems % channels == 0:
        return row_elems // channels
    p = row_elems // channels
    return p - p % 8 if p >= 8 else max(p, 1)


def affine_is_exact(src: torch.Tensor, scale, bias, plane: int | None) -> bool:
    """float64 ``x * s + b`` equals its float32 rounding for every element (channel from ``plane``, or from the
    last axis when ``plane`` is None)."""
    y = _affine64(src.reshape(src.shape[0], -1) if plane is not None else src, scale, bias, plane)
    return bool(torch.equal(y.float().double(), y))


def _affine64(x: torch.Tensor, scale, bias, plane):
    s = torch.tensor(_f32(scale), dtype=torch.float64)
    b = torch.tensor(_f32(bias), dtype=torch.float64)
    if plane is None:  # channel = last axis
        return x.double() * s + b
    ch = (torch.arange(x.shape[1]) // int(plane)) % len(scale)
    return x.double() * s[ch] + b[ch]


# ------------------------------------------------------------------ references
def _round(y64: torch.Tensor, out_dtype) -> torch.Tensor:
    return y64.float().to(out_dtype)  # one rounding to float32, then torch's CPU cast (RNE)


def ref_convert(src, rows, out_dtype, scale=None, bias=None, plane=None) -> torch.Tensor:
    """gather_rows: out[r] = cast(src[rows[r]] * scale[ch] + bias[ch]), ch = (elem // plane) % channels."""
    x = src[rows]
    if scale is None:
        if out_dtype == src.dtype:
            return x.clone()
        return _round(x.double(), out_dtype)
    flat = x.reshape(x.shape[0], -1)
    return _round(_affine64(flat, scale, bias, plane), out_dtype).reshape(x.shape)


def ref_collate(src_hwc, rows, out_dtype, scale=None, bias=None) -> torch.Tensor:
    """collate_hwc_to_chw: channel = last axis, moved to position 1."""
    x = src_hwc[rows]
    y = x.double() if scale is None else _affine64(x, scale, bias, None)
    return _round(y.movedim(-1, 1), out_dtype).contiguous()


def ref_split(src, rows, widths, out_dtype=None):
    x = src[rows]
    if out_dtype is not None and out_dtype != src.dtype:
        x = _round(x.double(), out_dtype)
    edges = np.concatenate([[0], np.cumsum(widths)])
    return tuple(x[:, a:b].contiguous() for a, b in zip(edges[:-1], edges[1:]))


def ref_pack(groups, rows, out_dtype=None):
    x = torch.cat([g[rows] for g in groups], dim=1)
    if out_dtype is not None and out_dtype != x.dtype:
        x = _round(x.double(), out_dtype)
    return x.contiguous()


# ----------------------------------------------------------------- comparisons
def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(_BITS[t.element_size()])


def _where(flat_idx, shape) -> str:
    row_len = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    return ", ".join(f"flat {i} = (row {i // row_len}, elem {i % row_len})" for i in flat_idx)


def assert_same(out: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    """Bit-equal wherever ``ref`` is not a NaN; a NaN (any payload) wherever it is."""
    assert out.dtype == ref.dtype, f"{what}: dtype {out.dtype} != {ref.dtype}"
    assert tuple(out.shape) == tuple(ref.shape), f"{what}: shape {tuple(out.shape)} != {tuple(ref.shape)}"
    o, r = out.detach().cpu(), ref
    ob, rb = _bits(o).reshape(-1), _bits(r).reshape(-1)
    if ref.is_floating_point():
        nan = torch.isnan(r).reshape(-1)
        bad = torch.where(nan, ~torch.isnan(o).reshape(-1), ob != rb)
    else:
        bad = ob != rb
    if bad.any():
        first = torch.nonzero(bad).reshape(-1)[:6].tolist()
        vals = [(o.reshape(-1)[i].item(), r.reshape(-1)[i].item(), hex(ob[i].item() & 0xFFFFFFFF),
                 hex(rb[i].item() & 0xFFFFFFFF)) for i in first]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at "
                             f"{_where(first, ref.shape)}; (out, ref, out bits, ref bits) = {vals}")


def _ordered(t: torch.Tensor) -> torch.Tensor:
    """Integers in the order of the floats they encode (-0 and +0 both map to 0)."""
    b = _bits(t).to(torch.int64)
    mag = b & ((1 << (8 * t.element_size() - 1)) - 1)
    return torch.where(b < 0, -mag, mag)


def assert_within_ulp(out: torch.Tensor, ref: torch.Tensor, ulps: int, what: str = "") -> None:
    """|out - ref| <= ``ulps`` units in the last place of the output dtype. For realistic affines only."""
    assert out.dtype == ref.dtype and tuple(out.shape) == tuple(ref.shape), what
    o = out.detach().cpu()
    assert torch.isfinite(o.float()).all() and torch.isfinite(ref.float()).all(), f"{what}: non-finite value"
    d = (_ordered(o) - _ordered(ref)).abs().reshape(-1)
    bad = d > ulps
    if bad.any():
        first = torch.nonzero(bad).reshape(-1)[:6].tolist()
        vals = [(o.reshape(-1)[i].item(), ref.reshape(-1)[i].item(), int(d[i])) for i in first]
        raise AssertionError(f"{what}: {int(bad.sum())} elements beyond {ulps} ulp, worst {int(d.max())}; first at "
                             f"{_where(first, ref.shape)}; (out, ref, ulps) = {vals}")


# ------------------------------------------------------------- dispatch mirror
def convert_path(in_dtype, out_dtype, row_elems, src_ptr, dst_ptr, plane=None) -> str:
    """Which kernel the host side of ``gather_rows`` launches (csrc/kernels/permute.hip): a mirror of its
    conditions, kept here so that a change of the dispatch that leaves a path untested fails the coverage
    assertion of test_kernel_refs.py."""
    if in_dtype == out_dtype and plane is None:
        return "move"
    vec_ok = row_elems % 8 == 0 and (src_ptr | dst_ptr) % 16 == 0
    if plane is not None and plane % 8 != 0:
        vec_ok = False
    if not (vec_ok and row_elems >= 256 * 8):
        return "flat"
    return "u8_chunked" if in_dtype == U8 else "chunked"


def move_unit(row_bytes, src_ptr, dst_ptr) -> int:
    """Bytes per lane access of a same-dtype move (16, 4 or 1)."""
    align = src_ptr | dst_ptr
    if row_bytes % 16 == 0 and align % 16 == 0:
        return 16
    return 4 if row_bytes % 4 == 0 and align % 4 == 0 else 1


# ------------------------------------------------------------- special values
def _f32_bits(v) -> int:
    return int(np.array(v, dtype=np.float32).view(np.uint32))


SPECIAL_F32_BITS = (
    0x7FC00000, 0xFFC00000,  # quiet NaNs
    0x7F800001, 0xFF800001, 0x7FBFFFFF, 0xFFFFFFFF,  # signalling NaNs of both signs, all-ones
    0x7F800000, 0xFF800000, 0x00000000, 0x80000000,  # +-inf, +-0
    0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF,  # smallest / largest subnormal
    0x7F7FFFFF, 0xFF7FFFFF,  # +-FLT_MAX: inf in bf16 and f16
    0x3F808000, 0x3F818000,  # bf16 ties, kept mantissa even / odd
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # their float32 neighbours
    _f32_bits(65504.0), _f32_bits(65519.99), _f32_bits(65520.0),  # f16 max, just below the tie to inf, the tie
    _f32_bits(2.0 ** -24), _f32_bits(2.0 ** -25), _f32_bits(2.0 ** -25) + 1,  # f16 subnormal, tie to 0, above it
)
SPECIAL_CHUNK = 8192  # elements per chunk of convert_rows_chunked for a float32 source
# 4 chunks: 4 last groups x 8 lanes hold every special value; one more element makes the row odd -> flat kernel
SPECIAL_ROW_ELEMS = {"chunked": 4 * SPECIAL_CHUNK, "flat": 4 * SPECIAL_CHUNK + 1}


def special_source(row_elems: int) -> tuple[torch.Tensor, list[list[int]]]:
    """[N_SRC, row_elems] float32 normal data; in every row special value j sits at lane 0 of 8-element group j,
    at lane 7 of group 64 + j, and in the last group of a chunk (chunk j // 8, lane j % 8). Returns the source
    and the three columns of each special value."""
    src = make_source(F32, (N_SRC, row_elems), "real", seed=77)
    cols = []
    for j, b in enumerate(SPECIAL_F32_BITS):
        c = [8 * j, 8 * (64 + j) + 7, (j // 8 + 1) * SPECIAL_CHUNK - 8 + j % 8]
        assert max(c) < row_elems and len(set(c)) == 3
        cols.append(c)
    flat = [c for cs in cols for c in cs]
    assert len(set(flat)) == len(flat)
    bits = src.view(torch.int32)
    for cs, b in zip(cols, SPECIAL_F32_BITS):
        bits[:, cs] = int(np.array(b, dtype=np.uint32).view(np.int32))
    return src, cols


# --------------------------------------------------------------- collate table
COLLATE_CHANNELS = (1, 2, 3, 4, 5, 8, 16)
COLLATE_IN = (U8, F32, BF16)
COLLATE_OUT = (BF16, F32)
# pixel counts around the generic kernel's 2048-pixel tile and the RGB kernel's 4096-pixel tile
COLLATE_HW = ((1, 1), (1, 7), (2, 4), (23, 89), (32, 64), (3, 683), (8, 257), (63, 65), (64, 64), (17, 241), (8, 513))
COLLATE_N_SRC, COLLATE_BATCH = 5, 3
assert [h * w for h, w in COLLATE_HW] == [1, 7, 8, 2047, 2048, 2049, 2056, 4095, 4096, 4097, 4104]


def collate_rows(how: str, seed: int) -> Rows:
    if how == "identity":
        return Rows(np.arange(1, 1 + COLLATE_BATCH), how, base=1)
    if how == "index":
        return Rows(np.array([COLLATE_N_SRC - 1, 0, COLLATE_N_SRC - 1]), how)
    p = FeistelPermutation(COLLATE_N_SRC, seed=seed + 1, epoch=1)
    return Rows(p(np.arange(2, 2 + COLLATE_BATCH, dtype=np.int64)), how, base=2, perm=p)


# ------------------------------------------------------------ split/pack table
SPLIT_N_SRC = 140
SPLIT_ROWS = (1, 7, 8, 9, 63, 64, 65)  # around the 8-row wave tile and the 64 lanes
SPLIT_VALUES = (1, 9, 255, 256, 257, 4096, 4097)  # around the 256-value switch of the row walk, the 4096 chunk
SPLIT_RAW = (U8, F16, I32, I64)  # 1-, 2-, 4- and 8-byte raw copies
SPLIT_CONVERT = ((U8, BF16), (U8, F32), (BF16, F32), (F32, BF16))


def split_groups(n_values: int) -> list[tuple[int, ...]]:
    g = [(n_values,)]
    if n_values >= 2:
        g.append((1, n_values - 1))
    if n_values >= 9:
        g.append((1,) * 7 + (n_values - 7,))
    return g


def split_rows(n_rows: int, how: str, seed: int) -> Rows:
    return rows_of(SPLIT_N_SRC, n_rows, how, seed)


# ------------------------------------------------------------------ move table
MOVE_DTYPES = (U8, F16, I32, I64, F32)
MOVE_ROW_BYTES = (16 * 255, 16 * 256, 16 * 1024, 16 * 1025, 4 * 255, 4 * 257, 1021)
MOVE_BYTE_OFFSETS = (4, 1)  # applied to 16-byte row sizes; an offset the element size does not divide becomes
#                             one element (int64: 8 bytes, f16 at 1: 2 bytes)


def move_cases():
    """(dtype, row_elems, offset_elems) with offset_elems in {0, offsets of 16-byte rows}."""
    out = []
    for dt in MOVE_DTYPES:
        es = torch.empty((), dtype=dt).element_size()
        for rb in MOVE_ROW_BYTES:
            if rb % es:
                continue
            offs = [0]
            if rb % 16 == 0:
                offs += sorted({max(o // es, 1) for o in MOVE_BYTE_OFFSETS})
            out.append((dt, rb // es, tuple(offs)))
    return out
