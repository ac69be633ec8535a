"""Every dispatch path of the row kernels (csrc/kernels/permute.hip) and the collate / split / pack kernels
(csrc/kernels/collate.hip) against independent float64 references (tests/kernel_refs.py).

The cases are those of tests/kernel_matrix.py, which tests/test_kernel_refs.py runs on the CPU first. Results
are bit-exact (``assert_same``) except under the realistic affine, where one fused multiply-add against a
float64 evaluation allows one ulp of the output dtype (``assert_within_ulp(.., 1)``; derivation in kernel_refs).
"""

import pytest
import torch

from ddl_amd import ops
from tests import kernel_matrix as M
from tests import kernel_refs as R
from tests.kernel_refs import BF16, F32, U8

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------ converting gather
@pytest.mark.parametrize("how", R.HOWS)
@pytest.mark.parametrize("row_elems", R.ROW_ELEMS)
def test_gather_cast(row_elems, how):
    """All cast pairs x grid caps {0, 1, 3}: flat below 2048 elements or off a multiple of 8, else chunked
    (8192-element chunks; 16384 for uint8 sources), at and 8 past each border."""
    M.run_gather_cast(row_elems, how, _dev())


@pytest.mark.parametrize("channels", R.AFFINE_CHANNELS)
@pytest.mark.parametrize("row_elems", R.ROW_ELEMS)
def test_gather_exact_affine(row_elems, channels):
    """1 / 3 / 4 channels (register select) and 5 / 16 (dynamic table load), every pair and addressing mode."""
    M.run_gather_affine(row_elems, channels, R.plane_for(row_elems, channels), _dev(), case=channels)


@pytest.mark.parametrize("row_elems,channels,plane", M.AFFINE_EXTRA)
def test_gather_affine_wrap_table_and_odd_plane(row_elems, channels, plane):
    """The % channels wrap inside a vector kernel (plane 8), a per-column table (plane 1, 16 channels) and a
    plane that is no multiple of 8 (flat kernel, per-element channel)."""
    M.run_gather_affine(row_elems, channels, plane, _dev())


@pytest.mark.parametrize("row_elems", M.REALISTIC_ROW_ELEMS)
def test_gather_realistic_affine(row_elems):
    M.run_gather_affine(row_elems, 3, row_elems // 3, _dev(), exact=False)


@pytest.mark.parametrize("side", ["src", "out"])
def test_gather_misaligned(side):
    M.run_gather_misaligned(side, _dev())


def test_cast_reshape():
    M.run_cast_reshape(_dev())


@pytest.mark.parametrize("kind", ["flat", "chunked"])
def test_gather_special_values(kind):
    """NaNs stay NaNs, infinities and zeros keep their sign, float32 subnormals are not flushed, ties go to even,
    in the scalar and in the packed conversions alike."""
    M.run_special_values(kind, _dev())


@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("row_elems", [2040, 16392])
def test_gather_from_host_rows(row_elems, max_blocks):
    """Zero-copy source (plain loads instead of non-temporal ones): u8 -> bf16 under the exact affine and
    f32 -> bf16, flat and chunked, uncapped and capped."""
    from ddl_amd import _native

    h = _native.hip()
    sc, bi = R.exact_affine(3)
    assert row_elems % 24 == 0  # three planes, each a multiple of 8: the long row reaches the chunked kernel
    for in_dt, affine in ((U8, (sc, bi, row_elems // 3)), (F32, (None, None, None))):
        host = R.make_source(in_dt, (R.N_SRC, row_elems), "real", seed=3)
        h.host_register(host.data_ptr(), host.numel() * host.element_size(), True)
        try:
            src = ops.HostRows(host, h.host_device_pointer(host.data_ptr()))
            for hi, how in enumerate(R.HOWS):
                rows = R.rows_of(R.N_SRC, R.n_gathered(hi), how, hi)
                out = ops.gather_rows(src, out_dtype=BF16, scale=affine[0], bias=affine[1], plane=affine[2],
                                      max_blocks=max_blocks, **rows.kw(_dev()))
                torch.cuda.synchronize()
                R.assert_same(out, R.ref_convert(host, rows.rows, BF16, *affine),
                              f"HostRows {R.name(in_dt)}->bf16 row={row_elems} {how} mb={max_blocks}")
        finally:
            torch.cuda.synchronize()
            h.host_unregister(host.data_ptr())


# ----------------------------------------------------------------------- moves
@pytest.mark.parametrize("dtype,row_elems,offsets", R.move_cases(),
                         ids=lambda v: R.name(v) if isinstance(v, torch.dtype) else None)
def test_moves(dtype, row_elems, offsets):
    """gather_rows / scatter_rows of 1- to 8-byte elements (int32 and int64 included) with the 16-, 4- and
    1-byte unit kernels picked by row size and by a misaligned source or destination."""
    M.run_moves(dtype, row_elems, offsets, _dev())


def test_row_index_is_validated():
    d = _dev()
    src = torch.zeros((R.N_SRC, 8), device=d)
    dst = torch.zeros((R.N_SRC, 8), device=d)
    idx = torch.arange(4, device=d)
    for op in (lambda i: ops.gather_rows(src, i), lambda i: ops.scatter_rows(dst, src[:i.numel()], i)):
        with pytest.raises(TypeError):
            op(idx.to(torch.int32))
        with pytest.raises(ValueError):
            op(idx.cpu())
        with pytest.raises(ValueError):
            op(torch.arange(8, device=d)[::2])
    with pytest.raises(ValueError):
        ops.scatter_rows(torch.zeros((R.N_SRC, 16), device=d)[:, ::2], src[:4], idx)  # dst is not contiguous
    with pytest.raises(ValueError):
        ops.scatter_rows(dst, torch.zeros((4, 8)), idx)  # source on the host
    with pytest.raises(ValueError):
        ops.gather_rows(src, idx, out=torch.zeros((4, 8)))  # out on the host


# --------------------------------------------------------------------- collate
@pytest.mark.parametrize("hw", R.COLLATE_HW, ids=lambda hw: f"{hw[0] * hw[1]}px")
@pytest.mark.parametrize("channels", R.COLLATE_CHANNELS)
def test_collate(channels, hw):
    """The generic LDS-tiled kernel for every channel count and source dtype (the uint8 RGB kernel at C == 3),
    with pixel counts a few pixels either side of their 2048- and 4096-pixel tiles."""
    M.run_collate(channels, hw, _dev())


@pytest.mark.parametrize("channels", [9, 16])
def test_collate_wide_f32_pixels(channels):
    """2048 pixels of 9 or 16 float32 channels are 72 / 128 KB, more LDS than a launch may request: the host
    shrinks the tile (1024 / 512 pixels) and the output is correct. Pixel counts around the smaller tiles."""
    for hw in ((1, 511), (1, 512), (3, 171), (1, 1025), (8, 257), (17, 241)):
        src = R.make_source(F32, (R.COLLATE_N_SRC, *hw, channels), "ints", seed=channels)
        sc, bi = R.exact_affine(channels)
        for hi, how in enumerate(R.HOWS):
            rows = R.collate_rows(how, seed=hi)
            for out_dt in R.COLLATE_OUT:
                out = ops.collate_hwc_to_chw(src.to(_dev()), out_dtype=out_dt, scale=sc, bias=bi, **rows.kw(_dev()))
                R.assert_same(out, R.ref_collate(src, rows.rows, out_dt, sc, bi),
                              f"collate f32 C={channels} hw={hw} ->{R.name(out_dt)} {how}")


def test_collate_out_is_validated():
    d = _dev()
    src = torch.zeros((R.COLLATE_N_SRC, 4, 6, 3), dtype=U8, device=d)
    good = torch.empty((R.COLLATE_N_SRC, 3, 4, 6), dtype=BF16, device=d)
    assert ops.collate_hwc_to_chw(src, out=good) is good
    for bad in (torch.empty_like(good, dtype=F32),  # dtype
                torch.empty((R.COLLATE_N_SRC, 3, 4, 7), dtype=BF16, device=d),  # element count
                torch.empty((R.COLLATE_N_SRC, 3, 4, 12), dtype=BF16, device=d)[..., ::2],  # contiguity
                torch.empty(good.shape, dtype=BF16)):  # device
        with pytest.raises(ValueError, match="out must be"):
            ops.collate_hwc_to_chw(src, out=bad)
    with pytest.raises(ValueError, match="contiguous"):
        ops.collate_hwc_to_chw(torch.zeros((R.COLLATE_N_SRC, 4, 6, 6), dtype=U8, device=d)[..., ::2])


# ------------------------------------------------------------------ split/pack
@pytest.mark.parametrize("n_values", R.SPLIT_VALUES)
@pytest.mark.parametrize("n_rows", R.SPLIT_ROWS)
def test_split_pack(n_rows, n_values):
    """split_columns / pack_columns and their round trip: 1, 2 and 8 groups, raw 1- to 8-byte copies and the
    four conversions, 8-row wave tiles that are partial, full and one row over, both row walks either side of
    256 values, and more than one 4096-value chunk."""
    M.run_split_pack(n_rows, n_values, _dev())
