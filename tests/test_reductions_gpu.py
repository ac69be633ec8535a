"""The reduction kernels of csrc/kernels/misc.hip (column_stats, the checksums, stream_copy, touch_pages)
against independent exact or float64 references (``tests/reduction_refs.py``, ``ops.ref_checksum``), one case
per dispatch path, with every output inside guard-filled memory."""

import numpy as np
import pytest
import torch

from ddl_amd import _native, ops
from tests import reduction_refs as R

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
ONES = 0xFFFFFFFF
# launch geometry of the checksum kernels (csrc/kernels/misc.hip): 256 threads, each 16 B per load and 8
# independent loads per unrolled pass (32 KiB per block and pass), at most 1024 blocks
CK_THREADS, CK_LOADS, CK_MAX_BLOCKS = 256, 8, 1024
BLOCK_SHARE = CK_THREADS * CK_LOADS * 16
CK_SIZES = (4, 12, 16, 20, BLOCK_SHARE - 4, BLOCK_SHARE, BLOCK_SHARE + 4, 8 * BLOCK_SHARE + 28,
            1024 * BLOCK_SHARE + 16 * 7 + 8)
GUARD64 = 0x5A5A5A5A5A5A5A5A


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------- column_stats
_worst = {}


@pytest.mark.parametrize("rows,cols", R.STATS_SHAPES)
def test_column_stats_every_path(rows, cols):
    """One shape per path of the narrow kernel (tail loop only, both loops, capped grid, one column, a column
    count that divides the block, one thread per column) and of the wide kernel (fewer rows than waves, partial
    and one-column last tiles, two row blocks), every kind of column in each: min / max bit for bit, mean and std
    within the bounds of ``reduction_refs.check_column_stats``. The wide kernel's cap of 1024 row blocks needs
    more than 4 M rows and is not reached here."""
    for start in R.kind_starts(cols):
        x = torch.tensor(R.stats_table(rows, cols, start), device=_dev())
        s = ops.column_stats(x)
        torch.cuda.synchronize()
        assert set(s) == {"sum", "sumsq", "min", "max", "mean", "std"}
        assert all(v.dtype == torch.float32 and v.shape == (cols,) and v.is_cuda for v in s.values())
        R.check_column_stats(s, R.stats_ref(rows, cols, start), [R.column_kind(j, start) for j in range(cols)],
                             report=_worst)
    print("worst error / bound so far (mean, std):", {str(k): [f"{v:.3g}" for v in w] for k, w in _worst.items()})


@pytest.mark.parametrize("offset,sd", R.RANDOM_KINDS[:4])
def test_column_stats_offset_columns(offset, sd):
    """The [20000, 9] offset + sd * randn tables of the CPU suite through the kernel."""
    x = R.offset_table(offset, sd)
    s = ops.column_stats(torch.tensor(x, device=_dev()))
    rep = {}
    try:
        R.check_column_stats(s, R.ref_column_stats(x), [(offset, sd)] * x.shape[1], report=rep)
    finally:
        print(f"offset {offset} sd {sd}: worst error / bound (mean, std) = {rep}")


def test_column_stats_writes_only_its_columns():
    """The native launcher adds into [cols] outputs: the elements around them keep their guard."""
    for rows, cols in [(7777, 9), (3000, 255), (999, 300)]:
        x = torch.tensor(R.stats_table(rows, cols), device=_dev())
        acc = torch.full((2, cols + 2), 7.0, dtype=torch.float64, device=_dev())
        mm = torch.full((2, cols + 2), 7.0, dtype=torch.float32, device=_dev())
        acc[:, 1:-1] = 0
        mm[0, 1:-1], mm[1, 1:-1] = float("inf"), float("-inf")
        _native.hip().column_stats(src=x.data_ptr(), n=rows, cols=cols, sum=acc[0, 1:].data_ptr(),
                                   sumsq=acc[1, 1:].data_ptr(), min=mm[0, 1:].data_ptr(), max=mm[1, 1:].data_ptr(),
                                   stream=_stream())
        torch.cuda.synchronize()
        assert (acc[:, [0, -1]] == 7.0).all() and (mm[:, [0, -1]] == 7.0).all()
        ref = R.stats_ref(rows, cols)
        assert torch.equal(mm[0, 1:-1].cpu(), torch.from_numpy(ref["min"].copy()))
        assert torch.equal(mm[1, 1:-1].cpu(), torch.from_numpy(ref["max"].copy()))
        d = R.stats_table(rows, cols).astype(np.float64)
        ok = [j for j in range(cols) if R.column_kind(j) != R.MINMAX_ONLY]
        np.testing.assert_allclose(acc[0, 1:-1].cpu().numpy()[ok], d.sum(0)[ok], rtol=1e-12, atol=1e-9)
        np.testing.assert_allclose(acc[1, 1:-1].cpu().numpy()[ok], (d * d).sum(0)[ok], rtol=1e-12)


@pytest.mark.parametrize("mode", ["standard", "minmax"])
def test_normalize_columns_offset_columns(mode):
    """normalize_columns on columns whose mean is up to 1e3 times their spread, against the reference harness's
    float64 normalisation; the tolerances apply to the normalised output, which is O(1)."""
    from ddl_amd.models.datasets import PointWiseData

    offsets = np.array([1000.0, -1000.0, 500.0, 0.0, 1.0, -3.0, 10.0, 100.0, 1000.0])
    raw = (offsets + np.random.default_rng(3).standard_normal((20_000, 9))).astype(np.float32)
    out = ops.normalize_columns(torch.from_numpy(raw).to(_dev()), mode, area_weighted=True).cpu().numpy()
    if mode == "standard":
        ref = PointWiseData.standard_normalize(raw.astype(np.float64), area_weighted=True)
        ref = np.concatenate([ref[0], ref[3][:, None]], 1)
    else:
        ref = PointWiseData.minmax_normalize(raw.astype(np.float64), 1, 2, 5, area_weighted=True)
        ref = np.concatenate([ref[0], ref[3][:, None]], 1)
        # the harness scales targets by max|x| instead of the half range: compare the parameter/x columns
        out, ref = out[:, :3], ref[:, :3]
    assert np.abs(ref).max() < 10
    np.testing.assert_allclose(out, ref, rtol=2e-4, atol=2e-4)


# ------------------------------------------------------------------- checksum
def _one_hot_positions(nbytes: int, blocks: int) -> list:
    """Word positions at every boundary of a checksum launch of ``blocks`` blocks over ``nbytes`` bytes."""
    n_words, n16 = nbytes // 4, nbytes // 16
    stride = blocks * CK_THREADS  # 16 B units per grid-stride step
    cand = [0, n_words - 1,              # first and last word
            4 * n16 - 1, 4 * n16,        # last word of the last full unit, first tail word
            4 * CK_THREADS - 1, 4 * CK_THREADS,          # either side of block 0's first 256 units
            BLOCK_SHARE // 4 - 1, BLOCK_SHARE // 4,      # either side of the first 32 KiB
            4 * stride - 1, 4 * stride,                  # either side of the first grid-stride step
            4 * CK_LOADS * stride - 1, 4 * CK_LOADS * stride]  # either side of the first unrolled pass
    return sorted({p for p in cand if 0 <= p < n_words})


def _checksum_blocks(nbytes: int) -> int:
    return min(max(-(-(nbytes // 16) // (CK_THREADS * CK_LOADS)), 1), CK_MAX_BLOCKS)


@pytest.mark.parametrize("nbytes", CK_SIZES)
def test_checksum_one_hot(nbytes):
    """Zeros and one all-ones word at each boundary of the launch (16 B unit, tail, block share, grid-stride
    step, unrolled pass; the last size reaches the 1024-block cap and a second pass): the sum is that word
    exactly, so a skipped or double-counted position shows."""
    x = torch.zeros(nbytes // 4, dtype=torch.int32, device=_dev())
    buf = torch.full((3,), GUARD64, dtype=torch.int64, device=_dev())
    for p in _one_hot_positions(nbytes, _checksum_blocks(nbytes)):
        x[p] = -1
        buf[1] = 0
        ops.checksum(x, out=buf[1:2])
        got = buf.tolist()
        assert got[1] & M64 == ONES, f"one-hot word {p} of {nbytes // 4}: {got[1] & M64:#x}"
        assert got[0] == got[2] == GUARD64
        x[p] = 0
    assert ops.checksum(x).item() == 0


def test_checksum_all_ones_and_accumulating_out():
    """Every word 0xFFFFFFFF (the u32 -> u64 widening at full magnitude), and ``out=`` adding modulo 2^64 across
    two calls from a start that makes the sum wrap."""
    nbytes = 8 * BLOCK_SHARE + 28
    x = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=_dev())
    ref = ops.ref_checksum(x)
    assert ref == (nbytes // 4) * ONES
    assert ops.checksum(x).item() & M64 == ref
    y = torch.randint(0, 256, (4096 * 5 + 12,), dtype=torch.uint8)
    buf = torch.full((3,), GUARD64, dtype=torch.int64, device=_dev())
    buf[1] = -5  # 2^64 - 5
    out = ops.checksum(x, out=buf[1:2])
    assert out.data_ptr() == buf[1:2].data_ptr()
    ops.checksum(y.to(_dev()), out=buf[1:2])
    got = buf.tolist()
    assert got[1] & M64 == ((1 << 64) - 5 + ref + ops.ref_checksum(y)) & M64
    assert ref + ops.ref_checksum(y) > 5  # the sum wrapped
    assert got[0] == got[2] == GUARD64


def test_checksum_drops_trailing_bytes():
    """A byte count that is no multiple of 4: the trailing 1..3 bytes are not part of the sum."""
    for nbytes in (4099, 4098, 4097, 7, 3):
        x = torch.randint(1, 256, (nbytes,), dtype=torch.uint8)
        ref = ops.ref_checksum(x)
        assert ref == ops.ref_checksum(x[:nbytes // 4 * 4])
        assert ops.checksum(x.to(_dev())).item() & M64 == ref


@pytest.mark.parametrize("n_partials", [1, 3, 1024])
@pytest.mark.parametrize("nbytes", [20, 8 * BLOCK_SHARE + 28])
def test_checksum_accumulator_one_hot(n_partials, nbytes):
    """ChecksumAccumulator with one block doing everything, three blocks, and 1024 mostly idle blocks: after k
    one-hot tensors the value is k words; reading it twice gives the same number, and the slots next to the
    partials keep their guard."""
    acc = ops.ChecksumAccumulator(_dev(), n_partials)
    buf = torch.full((n_partials + 2,), GUARD64, dtype=torch.int64, device=_dev())
    buf[1:-1] = 0
    acc.partials = buf[1:-1]
    x = torch.zeros(nbytes // 4, dtype=torch.int32, device=_dev())
    k = 0
    for p in _one_hot_positions(nbytes, n_partials):
        x[p] = -1
        acc.add(x)
        x[p] = 0
        k += 1
    assert acc.value() == k * ONES
    assert acc.value() == k * ONES
    assert buf[0].item() == buf[-1].item() == GUARD64
    assert int(buf[1:-1].sum().item()) == k * ONES


def test_checksum_argument_errors():
    """Host-side argument checks (nothing is launched): a pointer that is not 16 B aligned, no partials, too
    many partials."""
    base = torch.zeros(64, dtype=torch.uint8, device=_dev())
    view = base[4:36]
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    with pytest.raises(ValueError):
        ops.checksum(view)
    with pytest.raises(ValueError):
        ops.ChecksumAccumulator(_dev(), 4).add(view)
    for n in (0, CK_MAX_BLOCKS + 1):
        with pytest.raises(ValueError):
            ops.ChecksumAccumulator(_dev(), n).add(base)
    assert _native.hip().CHECKSUM_MAX_BLOCKS == CK_MAX_BLOCKS


# ---------------------------------------------------------------- stream_copy
COPY_SIZES = (16, 4096 - 16, 4 * 256 * 16 - 16, 4 * 256 * 16, 4 * 256 * 16 + 16, (1 << 20) + 48)


@pytest.mark.parametrize("blocks", [1, 3, 4096])
def test_stream_copy_is_bitwise(blocks):
    """The roofline probe moves every 16 B unit once: sizes around one block's unrolled pass (4 x 256 units), a
    tail, one block striding over everything and far more blocks than units; 64 guard bytes on each side of the
    destination stay."""
    hip = _native.hip()
    for nbytes in COPY_SIZES:
        src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=_dev())
        buf = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device=_dev())
        dst = buf[64:64 + nbytes]
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        hip.stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, blocks, _stream())
        torch.cuda.synchronize()
        assert torch.equal(dst, src), f"{nbytes} bytes, {blocks} blocks"
        assert (buf[:64] == 0xA5).all() and (buf[64 + nbytes:] == 0xA5).all()


def test_stream_copy_argument_errors():
    hip = _native.hip()
    src = torch.zeros(256, dtype=torch.uint8, device=_dev())
    dst = torch.full((256,), 0xA5, dtype=torch.uint8, device=_dev())
    for s, d, n in [(src.data_ptr(), dst.data_ptr(), 24), (src.data_ptr() + 4, dst.data_ptr(), 32),
                    (src.data_ptr(), dst.data_ptr() + 8, 32)]:
        with pytest.raises(ValueError):
            hip.stream_copy(s, d, n, 1, _stream())
    torch.cuda.synchronize()
    assert (dst == 0xA5).all()


# ---------------------------------------------------------------- touch_pages
PAGE, N_PAGES = 4096, 300
GUARD32 = 0x5A5A5A5A


def _page_words(n_pages=N_PAGES):
    i = np.arange(n_pages, dtype=np.uint64)
    return ((i * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _paged_tensor(words):
    host = np.zeros((len(words), PAGE // 4), dtype=np.uint32)
    host[:, 0] = words
    host[:, 1] = 0xDEAD0000 + np.arange(len(words))  # never read: a wrong offset shows
    return torch.from_numpy(host.view(np.int32)).to(_dev())


def _xor(a) -> int:
    return int(np.bitwise_xor.reduce(np.asarray(a, dtype=np.uint32))) if len(a) else 0


def _touch(t, nbytes, blocks):
    sink = torch.full((blocks + 2,), GUARD32, dtype=torch.int32, device=_dev())
    _native.hip().touch_pages(t.data_ptr(), nbytes, PAGE, sink[1:].data_ptr(), blocks, _stream())
    torch.cuda.synchronize()
    got = sink.cpu().numpy().view(np.uint32)
    assert got[0] == GUARD32 and got[-1] == GUARD32
    return got[1:-1]


@pytest.mark.parametrize("blocks", [1, 3, 64])
def test_touch_pages_blocks_and_range_end(blocks):
    """Device memory, several blocks: sink[b] is the xor of the first words of exactly the pages block b visits
    (page i belongs to block (i mod blocks * 256) // 256). A range that ends 4 bytes into the last page still
    reads it; one that ends 3 bytes into it does not."""
    words = _page_words()
    t = _paged_tensor(words)
    owner = (np.arange(N_PAGES) % (blocks * 256)) // 256
    for nbytes, n_read in [(N_PAGES * PAGE, N_PAGES), ((N_PAGES - 1) * PAGE + 4, N_PAGES),
                           ((N_PAGES - 1) * PAGE + 3, N_PAGES - 1), ((N_PAGES - 1) * PAGE, N_PAGES - 1)]:
        got = _touch(t, nbytes, blocks)
        want = [_xor(words[:n_read][owner[:n_read] == b]) for b in range(blocks)]
        assert got.tolist() == want, f"{nbytes} bytes"
        assert _xor(got) == _xor(words[:n_read])


def test_touch_pages_shorter_than_a_word_reads_nothing():
    """bytes in 1..3 hold no whole 4 B word: success without a launch, the sink keeps its guard."""
    t = _paged_tensor(_page_words(2))
    for nbytes in (0, 1, 2, 3):
        assert (_touch(t, nbytes, 2) == GUARD32).all()
    assert _touch(t, 4, 2).tolist() == [int(_page_words(2)[0]), 0]
