"""The row kernels (csrc/kernels/permute.hip) and the collate / split / pack kernels (csrc/kernels/collate.hip)
on sources and outputs past 2^32 bytes: every kernel shape and addressing mode at the rows around the byte
offsets 2^31 and 2^32, and an output of more than 2^32 units (the 64-bit branch of ``div_small``).

The sources are filled by position (tests/far_refs.py), so the expected rows are a formula evaluated on the CPU
and pushed through the references of tests/kernel_refs.py; nothing reads a big buffer back. Before each launch
the alias condition is asserted: the rows 2^31 and 2^32 bytes (and elements) in front of the rows a test reads
hold other values, so a 32-bit wrap, which stays inside the allocation and faults nothing, fails the comparison.
Everything is bit-exact.
"""

import numpy as np
import pytest
import torch

from ddl_amd import ops
from ddl_amd.permutation import FeistelPermutation
from tests import augment_refs as A
from tests import far_refs as FR
from tests import feistel_ref
from tests import kernel_refs as R
from tests.kernel_refs import BF16, F16, F32, U8

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


class _Big:
    """One BIG-byte device buffer, viewed per case; refilled only when a case needs another fill."""

    def __init__(self):
        self.buf = torch.empty(FR.BIG, dtype=U8, device=_dev())
        self.fill = None

    def table(self, dtype, row_elems: int, kind=None) -> torch.Tensor:
        es = torch.empty((), dtype=dtype).element_size()
        flat = self.buf.view(dtype)
        if self.fill != (dtype, kind):
            FR.fill_by_position(flat, kind)
            self.fill = (dtype, kind)
        n_src = flat.numel() // row_elems
        assert n_src * row_elems * es > 1 << 32
        return flat[:n_src * row_elems].view(n_src, row_elems)


@pytest.fixture(scope="module")
def big():
    FR.need_hbm(3 * FR.BIG)
    b = _Big()
    yield b
    b.buf = None
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big_dst():
    FR.need_hbm(3 * FR.BIG)
    b = [torch.empty(FR.BIG, dtype=U8, device=_dev())]
    yield b[0]
    b.clear()
    torch.cuda.empty_cache()


def _launches(how: str, row_bytes: int, n_src: int):
    """(rows, op keywords) of each launch of one addressing mode, the rows of ``mark_rows`` among them."""
    marks = FR.mark_rows(row_bytes, n_src)
    d = _dev()
    if how == "identity":  # 16 consecutive rows around each mark the table reaches
        for m in FR.MARKS:
            if m < n_src * row_bytes:
                base = min(FR.straddle_base(row_bytes, 16, m), n_src - 16)
                yield list(range(base, base + 16)), dict(base=base, n_rows=16)
    elif how == "index":
        yield marks, dict(index=torch.tensor(marks, dtype=torch.int64, device=d))
    else:  # three consecutive positions of a permutation of [0, n_src) around the one that maps to a mark row
        perm = FeistelPermutation(n_src, seed=11, epoch=3)
        for m in marks:
            base = min(max(feistel_ref.py_position(m, n_src, 11, 3) - 1, 0), n_src - 3)
            rows = [feistel_ref.py_perm(p, n_src, 11, 3) for p in range(base, base + 3)]
            assert m in rows
            yield rows, dict(perm=perm, base=base, n_rows=3)


# kernel, in dtype, out dtype, row elements, affine channels (0: none)
GATHER_SHAPES = (
    ("move_rows_chunked<u32x4>", U8, U8, 4096, 0),
    ("move_rows_flat<uint32_t>", U8, U8, 1000, 0),
    ("move_rows_flat<uint8_t>", U8, U8, 255, 0),
    ("convert_u8_rows_chunked", U8, BF16, 4096, 0),
    ("convert_rows_chunked", F32, BF16, 2048, 4),
    ("convert_rows_flat", F32, F16, 100, 0),
)


PATHS = {"move_rows_chunked": "move", "move_rows_flat": "move", "convert_u8_rows_chunked": "u8_chunked",
         "convert_rows_chunked": "chunked", "convert_rows_flat": "flat"}


@pytest.mark.parametrize("how", R.HOWS)
@pytest.mark.parametrize("kernel,in_dt,out_dt,row_elems,channels", GATHER_SHAPES, ids=[s[0] for s in GATHER_SHAPES])
def test_gather_rows_past_4gb(big, kernel, in_dt, out_dt, row_elems, channels, how):
    kind = None if in_dt == U8 else "ints"
    src = big.table(in_dt, row_elems, kind)
    n_src, es = src.shape[0], src.element_size()
    path = R.convert_path(in_dt, out_dt, row_elems, src.data_ptr(), 0, row_elems // channels if channels else None)
    assert path == PATHS[kernel.split("<")[0]]
    if path == "move":
        assert R.move_unit(row_elems * es, src.data_ptr(), 0) == {4096: 16, 1000: 4, 255: 1}[row_elems]
    affine = (None, None, None)
    if channels:
        affine = (*R.exact_affine(channels), row_elems // channels)
    seen_past = False
    for rows, kw in _launches(how, row_elems * es, n_src):
        FR.assert_no_alias([r * row_elems for r in rows], row_elems, in_dt, kind, es)
        exp_src = FR.expected_rows(rows, row_elems, in_dt, kind)
        if channels:
            assert R.affine_is_exact(exp_src, *affine)
        ref = R.ref_convert(exp_src, torch.arange(len(rows)), out_dt, *affine)
        out = ops.gather_rows(src, out_dtype=out_dt, scale=affine[0], bias=affine[1], plane=affine[2], **kw)
        torch.cuda.synchronize()
        R.assert_same(out, ref, f"{kernel} {how} rows {rows[:4]}..")
        seen_past |= max(rows) * row_elems * es >= 1 << 32
    assert seen_past


SCATTER_SHAPES = (("move_rows_chunked<u32x4>", 4096), ("move_rows_flat<uint32_t>", 1000),
                  ("move_rows_flat<uint8_t>", 255))


@pytest.mark.parametrize("kernel,row_bytes", SCATTER_SHAPES, ids=[s[0] for s in SCATTER_SHAPES])
def test_scatter_rows_past_4gb(big_dst, kernel, row_bytes):
    """64 rows scattered into a BIG-byte sentinel-filled destination at ``mark_rows``: the named rows hold the
    data, and every other byte (the rows next to them and those 2^31 and 2^32 bytes in front of them among them)
    still holds the sentinel."""
    n_dst = FR.BIG // row_bytes
    dst = FR.fill_value(big_dst, SENTINEL)[:n_dst * row_bytes].view(n_dst, row_bytes)
    rows = FR.mark_rows(row_bytes, n_dst, n_hashed=64)
    fixed = FR.mark_rows(row_bytes, n_dst, n_hashed=0)
    rows = sorted(set(fixed) | set([r for r in rows if r not in fixed][:64 - len(fixed)]))
    assert len(rows) == 64
    order = np.random.default_rng(5).permutation(64)
    index = torch.tensor(np.asarray(rows)[order], dtype=torch.int64)
    src = R.make_source(U8, (64, row_bytes), seed=21)
    assert R.move_unit(row_bytes, dst.data_ptr(), 0) == {4096: 16, 1000: 4, 255: 1}[row_bytes]
    ops.scatter_rows(dst, src.to(_dev()), index.to(_dev()))
    torch.cuda.synchronize()
    R.assert_same(dst[index.to(_dev())], src, f"{kernel}: scattered rows")
    flat = big_dst
    for r in rows:
        for nb in (r - 1, r + 1):
            if 0 <= nb < n_dst and nb not in rows:
                assert bool((dst[nb] == SENTINEL).all()), f"row {nb} next to {r} was written"
        for m in FR.MARKS[:2]:
            b0 = r * row_bytes - m
            if b0 >= 0:
                span = flat[b0:b0 + row_bytes]
                keep = torch.ones(row_bytes, dtype=torch.bool)
                for q in rows:  # bytes of that span that belong to another named row
                    lo, hi = max(q * row_bytes, b0), min((q + 1) * row_bytes, b0 + row_bytes)
                    if lo < hi:
                        keep[lo - b0:hi - b0] = False
                assert bool((span.cpu()[keep] == SENTINEL).all()), f"bytes {m} in front of row {r} were written"
    changed = sum(int((flat[c:c + FR.FILL_CHUNK] != SENTINEL).sum()) for c in range(0, FR.BIG, FR.FILL_CHUNK))
    assert changed == int((src != SENTINEL).sum()), "bytes outside the named rows were written"


# ------------------------------------------ output past 2^32 units: div_small
WIDE_ROWS, WIDE_ROW_BYTES, WIDE_SRC = 16_843_100, 255, 4099


def _wide_index():
    return (torch.arange(WIDE_ROWS, dtype=torch.int64, device=_dev()) * 7919) % WIDE_SRC


def _compare_slices(out, table, index, what):
    for r0 in range(0, WIDE_ROWS, FR.COMPARE_ROWS):
        r1 = min(r0 + FR.COMPARE_ROWS, WIDE_ROWS)
        ref = table.index_select(0, index[r0:r1])
        if not torch.equal(out[r0:r1].view(torch.uint8), ref.view(torch.uint8)):
            bad = (out[r0:r1].view(torch.uint8) != ref.view(torch.uint8)).nonzero()[0].tolist()
            raise AssertionError(f"{what}: rows {r0}..{r1} differ, first at (row, byte) {bad}")


def test_move_flat_output_past_2_32_units(big_dst):
    """move_rows_flat<uint8_t> with total_units > 2^32: ``div_small`` takes its 64-bit division."""
    assert WIDE_ROWS * WIDE_ROW_BYTES > 1 << 32 and WIDE_ROWS * WIDE_ROW_BYTES + 64 <= FR.BIG
    src = R.make_source(U8, (WIDE_SRC, WIDE_ROW_BYTES), seed=31).to(_dev())
    FR.fill_value(big_dst, SENTINEL)
    out = big_dst[:WIDE_ROWS * WIDE_ROW_BYTES].view(WIDE_ROWS, WIDE_ROW_BYTES)
    index = _wide_index()
    ops.gather_rows(src, index, out=out)
    torch.cuda.synchronize()
    _compare_slices(out, src, index, "move_rows_flat<uint8_t>")
    assert bool((big_dst[WIDE_ROWS * WIDE_ROW_BYTES:] == SENTINEL).all()), "bytes behind the output were written"


def test_convert_flat_output_past_2_32_elements():
    """convert_rows_flat u8 -> bf16 with total > 2^32 elements, against kernel_refs' conversion of the 4099 source
    rows, selected on the device slice by slice."""
    n = WIDE_ROWS * WIDE_ROW_BYTES
    FR.need_hbm(2 * n + (1 << 30))
    host = R.make_source(U8, (WIDE_SRC, WIDE_ROW_BYTES), seed=32)
    ref = R.ref_convert(host, torch.arange(WIDE_SRC), BF16).to(_dev())
    buf = torch.empty(n + 64, dtype=BF16, device=_dev())
    buf[n:] = R.GUARD
    out = buf[:n].view(WIDE_ROWS, WIDE_ROW_BYTES)
    index = _wide_index()
    ops.gather_rows(host.to(_dev()), index, out=out, out_dtype=BF16)
    torch.cuda.synchronize()
    _compare_slices(out, ref, index, "convert_rows_flat u8->bf16")
    assert bool((buf[n:] == R.GUARD).all()), "elements behind the output were written"
    del out, buf
    torch.cuda.empty_cache()


# --------------------------------------------------------------------- collate
@pytest.mark.parametrize("in_dt,c,hw", [(U8, 3, 64), (F32, 4, 16)], ids=["hwc3_u8", "generic_f32"])
def test_collate_past_4gb(big, in_dt, c, hw):
    """The specialised u8 RGB kernel and the generic kernel, batch = the images at ``mark_rows``."""
    kind = None if in_dt == U8 else "ints"
    row_elems = hw * hw * c
    table = big.table(in_dt, row_elems, kind)
    n_src, es = table.shape[0], table.element_size()
    src = table.view(n_src, hw, hw, c)
    rows = FR.mark_rows(row_elems * es, n_src, n_hashed=8)
    FR.assert_no_alias([r * row_elems for r in rows], row_elems, in_dt, kind, es)
    exp_src = FR.expected_rows(rows, row_elems, in_dt, kind).view(len(rows), hw, hw, c)
    sc, bi = R.exact_affine(c)
    for out_dt in (BF16, F32):
        ref = R.ref_collate(exp_src, torch.arange(len(rows)), out_dt, sc, bi)
        out = ops.collate_hwc_to_chw(src, torch.tensor(rows, dtype=torch.int64, device=_dev()), out_dtype=out_dt,
                                     scale=sc, bias=bi)
        torch.cuda.synchronize()
        R.assert_same(out, ref, f"collate {R.name(in_dt)} C={c} -> {R.name(out_dt)}")


# ------------------------------------------------------------------ split/pack
@pytest.mark.parametrize("n_values", [40, 5000], ids=["tile_walk", "long_row_walk"])
def test_split_and_pack_columns_past_4gb(big, n_values):
    """[n_src, 40] (the wave-tile walk) and [n_src, 5000] (the long-row walk) float32 past 2^32 bytes, rows at
    ``mark_rows``, raw and float32 -> bf16; pack_columns reads two views of the big buffer as its groups."""
    src = big.table(F32, n_values, "ints")
    n_src = src.shape[0]
    # a second group over the same buffer: rows one value narrower that end with the buffer, so its row r sits at
    # element off2 + r * w2; its rows around byte 2^32 join the batch
    flat, w2 = big.buf.view(F32), n_values - 1
    off2 = flat.numel() - n_src * w2
    second = flat[off2:].view(n_src, w2)
    cross2 = ((1 << 30) - off2) // w2
    rows = sorted(set(FR.mark_rows(n_values * 4, n_src)) | {cross2 - 1, cross2, cross2 + 1})
    assert 0 < cross2 < n_src - 1 and (off2 + cross2 * w2) * 4 <= 1 << 32 < (off2 + (cross2 + 1) * w2) * 4
    FR.assert_no_alias([r * n_values for r in rows], n_values, F32, "ints", 4)
    FR.assert_no_alias([off2 + r * w2 for r in rows], w2, F32, "ints", 4)
    exp_src = FR.expected_rows(rows, n_values, F32, "ints")
    at2 = np.asarray(rows, dtype=np.uint64).reshape(-1, 1) * np.uint64(w2) + np.uint64(off2) + np.arange(w2, dtype=np.uint64)
    exp_second = torch.from_numpy(FR.expected(at2, F32, "ints"))
    index = torch.tensor(rows, dtype=torch.int64, device=_dev())
    widths = (1, 7, n_values - 8)
    sel = torch.arange(len(rows))
    for out_dt in (None, BF16):
        outs = ops.split_columns(src, widths, index, out_dtype=out_dt)
        torch.cuda.synchronize()
        for o, r in zip(outs, R.ref_split(exp_src, sel, widths, out_dt)):
            R.assert_same(o, r, f"split_columns {n_values} -> {out_dt}")
        out = ops.pack_columns([src, second], index, out_dtype=out_dt)
        torch.cuda.synchronize()
        R.assert_same(out, R.ref_pack([exp_src, exp_second], sel, out_dt), f"pack_columns {n_values} -> {out_dt}")


# ------------------------------------------------------------------------ crop
CROP_HW, CROP_SEED, CROP_BASE = (64, 64), 13, (1 << 33) + 5


def _crop_source(big):
    row_elems = 3 * CROP_HW[0] * CROP_HW[1]
    table = big.table(U8, row_elems)
    n_src = table.shape[0]
    rows = FR.mark_rows(row_elems, n_src, n_hashed=8)
    FR.assert_no_alias([r * row_elems for r in rows], row_elems, U8, None, 1)
    exp = FR.expected_rows(rows, row_elems, U8).view(len(rows), 3, *CROP_HW)
    return table.view(n_src, 3, *CROP_HW), rows, exp


def _impls(src, out_hw):
    """Every ``path`` of the launcher; ``lds`` only where a band fits its budget (it raises otherwise)."""
    return [i for i in A.EXACT_IMPLS if i != "lds" or A.rrc_path(U8, "chw", 3, CROP_HW, out_hw, src.data_ptr(), i).fits]


@pytest.mark.parametrize("out_hw", [(64, 64), (32, 32)], ids=["same", "half"])
def test_crop_whole_images_past_4gb(big, out_hw):
    """Whole-image crops (weights 0 and 1/2) of the images at ``mark_rows`` under the exact affine: bit-exact for
    float32 and bfloat16 output on every path."""
    src, rows, exp = _crop_source(big)
    sc, bi, mean, std = A.affine_of(3, U8, exact=True)
    whole = A.whole_image_kw(CROP_HW)
    boxes, amb = A.ref_boxes(np.asarray(rows), CROP_HW, seed=CROP_SEED, sample_base=CROP_BASE, **whole)
    assert not bool(amb.any())
    ref = A.ref_resample(exp, torch.arange(len(rows)), boxes, out_hw, "chw", F32, sc, bi)
    assert torch.equal(ref.value, ref.value.float().double())
    index = torch.tensor(rows, dtype=torch.int64, device=_dev())
    impls = _impls(src, out_hw)
    assert "auto" in impls and "direct" in impls
    for impl in impls:
        for out_dt, want in ((F32, ref.out), (BF16, R._round(ref.value, BF16))):
            out, b = ops.random_resized_crop(src, index, size=out_hw, out_dtype=out_dt, return_boxes=True, impl=impl,
                                             seed=CROP_SEED, sample_base=CROP_BASE, mean=mean, std=std, **whole)
            assert torch.equal(b.cpu(), boxes), impl
            R.assert_same(out, want, f"whole-image crop {out_hw} {impl} {R.name(out_dt)}")


def test_random_crops_past_4gb(big):
    """Random crops keyed by ``sample_base`` + source row (keys past 2^33): the boxes equal ``ref_boxes`` on every
    unambiguous image, the float32 pixels lie within augment_refs' derived bound of the float64 resampling of the
    formula's images, and the bfloat16 output is the RNE bfloat16 of the float32 one, on every path."""
    src, rows, exp = _crop_source(big)
    out_hw = (24, 40)
    sc, bi, mean, std = A.affine_of(3, U8)
    boxes, amb = A.ref_boxes(np.asarray(rows), CROP_HW, seed=CROP_SEED, sample_base=CROP_BASE)
    assert float(amb.double().mean()) <= A.MAX_AMBIGUOUS
    ref = A.ref_resample(exp, torch.arange(len(rows)), boxes, out_hw, "chw", F32, sc, bi)
    index = torch.tensor(rows, dtype=torch.int64, device=_dev())
    kw = dict(size=out_hw, return_boxes=True, seed=CROP_SEED, sample_base=CROP_BASE, mean=mean, std=std)
    for impl in _impls(src, out_hw):
        out32, b = ops.random_resized_crop(src, index, out_dtype=F32, impl=impl, **kw)
        assert not bool(((b.cpu() != boxes).any(1) & ~amb).any()), f"{impl}: boxes differ from ref_boxes"
        A.assert_resampled(out32, ref, f"random crop {impl}", ~amb)
        out16, _ = ops.random_resized_crop(src, index, out_dtype=BF16, impl=impl, **kw)
        A.assert_bf16_of(out16, out32, f"random crop {impl}")


# ------------------------------------------------------------ launcher refusals
def test_tile_count_refusals_are_raised():
    """Shapes whose tile count does not fit the kernels' 32-bit tile arithmetic are refused by the launchers (code
    -4) before anything is launched or read: 2^30 rows of 513 int64 are 2^31 tiles of ``move_rows_chunked`` and pass
    ``gather_rows``' other bounds; 2^20 RGB images of 2^24 pixels are 2^32 tiles of the u8 collate. The pointers are
    a small real allocation that is never touched."""
    from ddl_amd import _native

    hip = _native.hip()
    buf = torch.zeros(4096, dtype=torch.uint8, device=_dev())
    sel = ops.row_selector(None, None, 0)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(ValueError, match=r"-4"):
        hip.gather_rows(dst=buf.data_ptr(), out_dt=2, src=buf.data_ptr(), in_dt=2, n_rows=1 << 30, row_elems=513,
                        scale=[], bias=[], plane=0, scatter=False, stream=st, max_blocks=0, host_src=False, **sel)
    with pytest.raises(ValueError, match=r"-4"):
        hip.collate_hwc_to_chw(dst=buf.data_ptr(), out_dt=4, src=buf.data_ptr(), in_dt=0, batch=1 << 20,
                               pixels=1 << 24, channels=3, scale=[], bias=[], stream=st, **sel)
    torch.cuda.synchronize()
    assert not bool(buf.any())
