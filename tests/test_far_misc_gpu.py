"""The permutation, owner-bucketing and reduction kernels (csrc/kernels/permute.hip feistel_fill,
csrc/kernels/bucket.hip, csrc/kernels/misc.hip) past the 32-bit marks: a Feistel domain of 2^33 + 12345 rows
(half_bits 17), checksums, copies and page touches over 2^32 + 2^20 + 12 bytes, and column statistics of a table
of more than 2^32 elements. Position-filled inputs (tests/far_refs.py); the references are the scalar Feistel
network in Python integers, ``tests/reduction_refs.py`` and chunked torch sums in int64 / float64."""

import numpy as np
import pytest
import torch

from ddl_amd import _native, ops
from ddl_amd.permutation import FeistelPermutation
from tests import far_refs as FR
from tests import feistel_ref
from tests import reduction_refs as R

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
GUARD = -(0x5A5A5A5A5A5A5A5A)
GUARD32 = 0x5A5A5A5A

FAR_N = (1 << 33) + 12345
FAR_SEED, FAR_EPOCH = 9, 2
FAR_COUNT = 4096
FAR_BASES = (0, (1 << 32) - 100, FAR_N - FAR_COUNT)
WORLD = 8


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return torch.cuda.current_stream().cuda_stream


_far_perm_cache = {}


def _far_perm(base: int) -> np.ndarray:
    """perm(base .. base + 4096) of the far domain from the scalar reference, computed once per base."""
    if base not in _far_perm_cache:
        v = np.array([feistel_ref.py_perm(p, FAR_N, FAR_SEED, FAR_EPOCH) for p in range(base, base + FAR_COUNT)],
                     dtype=np.int64)
        v.setflags(write=False)
        _far_perm_cache[base] = v
    return _far_perm_cache[base]


class _ScalarPerm:
    """The scalar reference behind the ``numpy_eval`` surface ``reduction_refs.ref_owner_maps`` asks of a
    permutation, for the positions base .. base + 4096 only (batch 0 of the oracle = those positions)."""

    def __init__(self, base):
        self.base = base

    def numpy_eval(self, pos):
        assert pos[0] == 0 and len(pos) == FAR_COUNT
        return _far_perm(self.base).copy()


@pytest.mark.parametrize("base", FAR_BASES)
def test_feistel_indices_far_domain(base):
    px = FeistelPermutation(FAR_N, FAR_SEED, FAR_EPOCH)
    assert px.half_bits == 17
    ref = _far_perm(base)
    assert ref.max() > 1 << 32 and ref.min() >= 0 and ref.max() < FAR_N
    buf = torch.full((FAR_COUNT + 16,), GUARD, dtype=torch.int64, device=_dev())
    _native.hip().feistel_indices(out=buf[8:].data_ptr(), count=FAR_COUNT, base=base, stream=_stream(),
                                  **px.device_args())
    got = buf.cpu().numpy()
    assert np.array_equal(got[8:-8], ref)
    assert (got[:8] == GUARD).all() and (got[-8:] == GUARD).all()
    assert np.array_equal(ops.feistel_indices(px, base, FAR_COUNT, device=_dev()).cpu().numpy(), ref)
    assert np.array_equal(px(np.arange(base, base + FAR_COUNT, dtype=np.int64)), ref)  # the host twin


@pytest.mark.parametrize("base", FAR_BASES)
def test_bucketing_far_domain(base):
    """World 8, shard_rows = ceil(n / 8) > 2^30: every rank's send list and receive map of the 4096 positions from
    ``base`` against the numpy oracle fed by the scalar permutation."""
    hip = _native.hip()
    px = FeistelPermutation(FAR_N, FAR_SEED, FAR_EPOCH)
    gb, lb, shard = FAR_COUNT, FAR_COUNT // WORLD, -(-FAR_N // WORLD)
    oracle = _ScalarPerm(base)
    sent = 0
    for rank in range(WORLD):
        ref_send, ref_inv, ref_sc, ref_rc = R.ref_owner_maps(oracle, FAR_N, 0, gb, WORLD, rank)
        n_send = len(ref_send)
        sent += n_send
        send = torch.full((gb + 8,), GUARD, dtype=torch.int64, device=_dev())
        inv = torch.full((lb + 8,), GUARD, dtype=torch.int64, device=_dev())
        hip.bucket_send(px.keys, FAR_N, px.half_bits, base, gb, shard, rank * shard, rank, WORLD, send.data_ptr(),
                        _stream())
        offs = np.concatenate([[0], np.cumsum(ref_rc)[:-1]]).tolist()
        hip.bucket_recv(px.keys, FAR_N, px.half_bits, base + rank * lb, lb, shard, WORLD, offs, inv.data_ptr(),
                        _stream())
        send, inv = send.cpu().numpy(), inv.cpu().numpy()
        where = f"base {base} rank {rank}"
        assert np.array_equal(send[:n_send], ref_send), where
        assert (send[n_send:] == GUARD).all(), where
        assert np.array_equal(inv[:lb], ref_inv), where
        assert (inv[lb:] == GUARD).all(), where
    assert sent == gb


# ------------------------------------------------ checksum / copy / touch pages
FAR_BYTES = FR.BIG + 12


@pytest.fixture(scope="module")
def far_words():
    FR.need_hbm(3 * FAR_BYTES)
    hold = [FR.fill_by_position(torch.empty(FAR_BYTES // 4, dtype=torch.int32, device=_dev()))]
    yield hold[0]
    hold.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def far_word_sum(far_words):
    """Sum of the 32-bit words modulo 2^64: torch int64 sums of the zero-extended words, chunk by chunk."""
    total = 0
    for c in range(0, far_words.numel(), FR.FILL_CHUNK):
        total += int((far_words[c:c + FR.FILL_CHUNK].to(torch.int64) & 0xFFFFFFFF).sum().item())
    return total & M64


def test_checksum_past_4gb(far_words, far_word_sum):
    assert far_words.numel() * 4 == FAR_BYTES and FAR_BYTES % 16 == 12
    probe = np.array([0, 1 << 29, 1 << 30, far_words.numel() - 1], dtype=np.uint64)  # words at bytes 0, 2^31, 2^32
    at = torch.from_numpy(probe.astype(np.int64)).to(_dev())
    assert far_words[at].cpu().numpy().tolist() == FR.expected(probe, torch.int32).tolist()
    buf = torch.full((3,), GUARD, dtype=torch.int64, device=_dev())
    buf[1] = 0
    ops.checksum(far_words, out=buf[1:2])
    got = buf.tolist()
    assert got[1] & M64 == far_word_sum
    assert got[0] == got[2] == GUARD


@pytest.mark.parametrize("n_partials", [3, 1024])
def test_checksum_accumulator_past_4gb(far_words, far_word_sum, n_partials):
    acc = ops.ChecksumAccumulator(_dev(), n_partials)
    acc.add(far_words)
    assert acc.value() == far_word_sum
    acc.add(far_words)
    assert acc.value() == (2 * far_word_sum) & M64


@pytest.mark.parametrize("blocks", [3, 4096])
def test_stream_copy_past_4gb(far_words, blocks):
    nbytes = FAR_BYTES // 16 * 16
    assert nbytes > 1 << 32
    src = far_words.view(torch.uint8)
    buf = torch.empty(nbytes + 128, dtype=torch.uint8, device=_dev())
    FR.fill_value(buf, 0xA5)
    dst = buf[64:64 + nbytes]
    _native.hip().stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, blocks, _stream())
    torch.cuda.synchronize()
    for c in range(0, nbytes, FR.FILL_CHUNK):
        assert torch.equal(dst[c:c + FR.FILL_CHUNK], src[c:min(c + FR.FILL_CHUNK, nbytes)]), f"bytes from {c}"
    assert bool((buf[:64] == 0xA5).all()) and bool((buf[64 + nbytes:] == 0xA5).all())
    del dst, buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("page", [4096, 1 << 31])
@pytest.mark.parametrize("blocks", [3, 64])
def test_touch_pages_past_4gb(far_words, blocks, page):
    """sink[b] is the xor of the first words of the pages block b visits (page i belongs to block
    (i mod blocks * 256) // 256), as in tests/test_reductions_gpu.py; the words come from the fill formula."""
    n_pages = (FAR_BYTES - 4) // page + 1
    assert (n_pages - 1) * page >= 1 << 32
    words = FR.expected(np.arange(n_pages, dtype=np.uint64) * np.uint64(page // 4), torch.int32).view(np.uint32)
    owner = (np.arange(n_pages) % (blocks * 256)) // 256
    want = [int(np.bitwise_xor.reduce(words[owner == b])) if (owner == b).any() else 0 for b in range(blocks)]
    sink = torch.full((blocks + 2,), GUARD32, dtype=torch.int32, device=_dev())
    _native.hip().touch_pages(far_words.data_ptr(), FAR_BYTES, page, sink[1:].data_ptr(), blocks, _stream())
    torch.cuda.synchronize()
    got = sink.cpu().numpy().view(np.uint32)
    assert got[0] == GUARD32 and got[-1] == GUARD32
    assert got[1:-1].tolist() == want


# --------------------------------------------------------------- column_stats
STATS_ROWS, STATS_COLS = 477_218_700, 9


def test_column_stats_narrow_past_2_32_elements():
    """The narrow kernel over n * cols > 2^32 elements of N(3, 1)-like values. Reference: float64 sums per column
    by torch, chunk by chunk (two passes: the mean, then the spread about it; exact min / max); bound: exactly
    ``reduction_refs.check_column_stats`` for this table."""
    assert STATS_ROWS * STATS_COLS > 1 << 32
    FR.need_hbm(40 << 30)
    x = FR.fill_by_position(torch.empty((STATS_ROWS, STATS_COLS), dtype=torch.float32, device=_dev()), "normal")
    s = ops.column_stats(x)
    torch.cuda.synchronize()
    step = 1 << 24
    tot = torch.zeros(STATS_COLS, dtype=torch.float64, device=_dev())
    mn = torch.full((STATS_COLS,), float("inf"), device=_dev())
    mx = -mn
    for r in range(0, STATS_ROWS, step):
        c = x[r:r + step]
        tot += c.double().sum(0)
        mn, mx = torch.minimum(mn, c.min(0).values), torch.maximum(mx, c.max(0).values)
    mean = tot / STATS_ROWS
    dev2 = torch.zeros_like(tot)
    for r in range(0, STATS_ROWS, step):
        dev2 += ((x[r:r + step].double() - mean) ** 2).sum(0)
    mean, std = mean.cpu().numpy(), torch.sqrt(dev2 / STATS_ROWS).cpu().numpy()
    ref = {"mean": mean, "std": std, "min": mn.cpu().numpy(), "max": mx.cpu().numpy(), "ulp_mean": R.ulp32(mean),
           "ulp_floor": R.ulp32(np.abs(mean) + np.abs(std))}
    assert np.all(np.abs(mean - 3) < 0.01) and np.all(np.abs(std - 1) < 0.01)
    rep = {}
    try:
        R.check_column_stats(s, ref, [(3.0, 1.0)] * STATS_COLS, report=rep)
    finally:
        print(f"[{STATS_ROWS}, {STATS_COLS}]: worst error / bound (mean, std) = {rep}")
    del x
    torch.cuda.empty_cache()
