"""``ops.gather_stream_pieces`` against ``ops.ref_gather_stream_pieces`` and against the stream itself, bitwise, over
plans the ``token_stream_plan`` kernel wrote."""

import numpy as np
import pytest
import torch

from ddl_amd import _native, ops

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = -7  # what the plan arrays hold where the plan kernel wrote nothing


def _tokens(np_dtype, n, seed):
    info = np.iinfo(np_dtype)
    return np.random.default_rng(seed).integers(info.min, info.max, size=n, dtype=np_dtype, endpoint=True)


def _source(toks: np.ndarray, kind: str):
    if kind == "device":
        return torch.from_numpy(toks).cuda(), None
    cpu = torch.from_numpy(toks).pin_memory()  # pinned and device-mapped
    return ops.HostRows(cpu, _native.hip().host_device_pointer(cpu.data_ptr())), cpu


def _plan(offs: np.ndarray, S: int, rows: int, row_base: int, max_segs: int):
    """(seg_src, seg_offsets, counts) of rows [row_base, row_base + rows) of the unshuffled stream, by the kernel."""
    dev_offs = torch.from_numpy(offs).cuda()
    n = offs.size - 1
    table = ops.token_stream_table(dev_offs)
    seg_src = torch.full((max_segs,), FILL, dtype=torch.int64, device="cuda")
    seg_offsets = torch.full((max_segs + 1,), FILL, dtype=torch.int64, device="cuda")
    rs, re = (torch.empty(rows, dtype=torch.int64, device="cuda") for _ in range(2))
    counts = torch.empty(4, dtype=torch.int64, device="cuda")
    _native.hip().token_stream_plan(
        table=table.data_ptr(), corpus_offsets=dev_offs.data_ptr(), n_corpus=n, n=n, row_base=row_base, rows=rows,
        seq_len=S, max_segs=max_segs, seg_offsets=seg_offsets.data_ptr(), seg_src=seg_src.data_ptr(),
        row_start=rs.data_ptr(), row_end=re.data_ptr(), counts=counts.data_ptr(),
        stream=torch.cuda.current_stream().cuda_stream, **ops.row_selector())
    return seg_src, seg_offsets, counts


def _check(src, toks, offs, S, rows, row_base, max_blocks, max_segs=None):
    """The window's tokens are the stream's (the corpus in document order: empty documents add nothing), what lies
    past them and on both sides of the window keeps the sentinel, and the reference says the same."""
    n_win = rows * S
    T = int(offs[-1])
    M = n_win + rows if max_segs is None else max_segs  # no window holds more pieces than tokens + row cuts
    seg_src, seg_offsets, counts = _plan(offs, S, rows, row_base, M)
    sentinel = 0x5A5A if toks.dtype.itemsize == 2 else 0x5A5A5A5A
    full = torch.full((GUARD + n_win + GUARD,), sentinel, dtype=torch.from_numpy(toks[:1]).dtype, device="cuda")
    out = ops.gather_stream_pieces(src, seg_src, seg_offsets, counts, rows, S, out=full[GUARD:GUARD + n_win],
                                   max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert out.data_ptr() == full[GUARD:].data_ptr() and out.numel() == n_win
    host = full.cpu().numpy()
    want = np.full(n_win, sentinel, dtype=toks.dtype)
    c = counts.cpu().numpy()
    n_tok = max(0, min(T - row_base * S, n_win))
    if max_segs is None:  # a plan that fits: every token of the window
        assert c[0] == -(-n_tok // S) and c[2] == n_tok
        want[:n_tok] = toks[row_base * S:row_base * S + n_tok]
    else:  # overflowed: the window stays untouched
        assert c[0] == -1 and c[1] > max_segs
    assert np.array_equal(host[GUARD:GUARD + n_win], want)
    assert (host[:GUARD] == sentinel).all() and (host[GUARD + n_win:] == sentinel).all()
    ref = ops.ref_gather_stream_pieces(torch.from_numpy(toks), seg_src, seg_offsets, counts, rows, S,
                                       out=torch.full((n_win,), sentinel, dtype=out.dtype))
    assert torch.equal(out.cpu(), ref)
    return int(c[1])


def _corpus(S, np_dtype):
    """Documents of 0, 1, S and 3 S + 1 tokens between fillers whose lengths walk the start's residue modulo 8."""
    lens = []
    for i in range(6):
        lens += [0, 1, i % 8, S, 3 * S + 1, (3 * i + 1) % 8, 0, 1, 1]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return _tokens(np_dtype, int(offs[-1]), 5), offs


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("S", [4, 60, 64])
@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_gather_matches_the_reference_bitwise(np_dtype, kind, S, rows):
    toks, offs = _corpus(S, np_dtype)
    src, _keep = _source(toks, kind)
    stream_rows = int(offs[-1]) // S
    segs = set()
    for row_base in (0, 1, 5, stream_rows // 2, stream_rows - rows + 1, stream_rows + 2):
        # the last two reach past the stream's end: a partial window, and one with no token at all
        segs.add(_check(src, toks, offs, S, rows, row_base, 0))
    assert 0 in segs and max(segs) > rows  # the empty window made no piece, others several per row
    # a capacity the window overflows: counts[0] = -1, nothing is read or written
    _check(src, toks, offs, S, rows, 0, 0, max_segs=1)


@pytest.mark.parametrize("max_blocks", [0, 1])
@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_gather_windows_of_several_chunks(np_dtype, kind, max_blocks):
    """400 rows of 64 tokens are 3.1 chunks of 16-bit ids and 6.3 of 32-bit ones: chunk boundaries inside pieces,
    one workgroup striding over all the chunks (``max_blocks=1``) and one workgroup per chunk."""
    chunk = _native.hip().STREAM_GATHER_CHUNK_BYTES // np.dtype(np_dtype).itemsize
    lens = np.random.default_rng(11).integers(0, 300, size=220)
    lens[::7] = 1  # runs of the shortest documents among them
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows, S = 400, 64
    assert offs[-1] > rows * S > 2 * chunk
    toks = _tokens(np_dtype, int(offs[-1]), 9)
    src, _keep = _source(toks, kind)
    _check(src, toks, offs, S, rows, 3, max_blocks)


def test_gather_refuses_bad_arguments():
    toks, offs = _corpus(64, np.int16)
    src = torch.from_numpy(toks).cuda()
    seg_src, seg_offsets, counts = _plan(offs, 64, 2, 0, 64)
    with pytest.raises(TypeError, match="2- or 4-byte"):
        ops.gather_stream_pieces(src.to(torch.int64), seg_src, seg_offsets, counts, 2, 64)
    with pytest.raises(TypeError, match="int64"):
        ops.gather_stream_pieces(src, seg_src.to(torch.int32), seg_offsets, counts, 2, 64)
    with pytest.raises(ValueError, match="bad out"):
        ops.gather_stream_pieces(src, seg_src, seg_offsets, counts, 2, 64, out=torch.empty(100, dtype=torch.int16,
                                                                                           device="cuda"))
    with pytest.raises(ValueError, match="GPU"):
        ops.gather_stream_pieces(src, seg_src.cpu(), seg_offsets, counts, 2, 64)
