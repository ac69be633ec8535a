"""The token kernels on corpora past the 32-bit marks (csrc/kernels/ragged.hip, csrc/kernels/tokens_indexed.hip):
a 2-byte corpus of 2^32 + 2^20 tokens and a 4-byte corpus of 2^31 + 2^20 tokens, about 8.6 GB each and live one at
a time, with sequences across every byte and element mark, the usual short lengths next to them and the last
sequence of the corpus. The corpus is filled by position (tests/far_refs.py); the references are the CPU
references of ``ddl_amd.ops`` run on the few thousand tokens the formula gives for the selected sequences. All
comparisons are bit-exact, and the alias condition (other tokens 2^31 and 2^32 bytes and elements in front of
every sequence read) is asserted before the launches."""

import numpy as np
import pytest
import torch

from ddl_amd import _native, ops
from tests import far_refs as FR

pytestmark = pytest.mark.gpu

PAD_ID = -3
LONG = 5000
SHORT = (0, 1, 7, 8, 9)
SENTINEL = 0x5A5A
CORPORA = {"u16": (torch.int16, (1 << 32) + (1 << 20)), "i32": (torch.int32, (1 << 31) + (1 << 20))}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _layout(dtype, n_elems):
    """(corpus_offsets, idx): sequences of interest at the odd positions of the offsets, unselected filler between
    them. One 5000-token sequence at an odd start near the corpus's beginning, one across each byte and element
    mark inside the corpus, the short lengths 11 tokens apart behind each, and the corpus's last 5000 tokens."""
    eb = torch.empty((), dtype=dtype).element_size()
    marks = sorted({m // eb for m in FR.MARKS} | set(FR.MARKS))
    seqs = [(5, LONG)]
    for m in marks:
        if m + LONG < n_elems - LONG:
            s = m - 5  # the mark inside the first row of every seq_len used: pad mode reads it too
            seqs.append((s, LONG))
            at = s + LONG + 11
            for ln in SHORT:
                seqs.append((at, ln))
                at += ln + 11
    seqs.append((n_elems - LONG, LONG))
    offs = [0]
    for s, ln in seqs:
        assert s > offs[-1]
        offs += [s, s + ln]
    if offs[-1] != n_elems:
        offs.append(n_elems)
    idx = np.arange(1, 2 * len(seqs), 2)
    order = np.random.default_rng(3).permutation(len(idx))
    return np.asarray(offs, dtype=np.int64), idx[order], eb


@pytest.fixture(scope="module", params=list(CORPORA))
def corpus(request):
    dtype, n = CORPORA[request.param]
    offs, idx, eb = _layout(dtype, n)
    starts, lens = offs[idx], offs[idx + 1] - offs[idx]
    assert starts.max() + LONG == n and (starts * eb > 1 << 32).any()
    for s, ln in zip(starts.tolist(), lens.tolist()):
        if ln:
            FR.assert_no_alias([s], ln, dtype, None, eb)
    FR.need_hbm(int(1.5 * n * eb))
    hold = [FR.fill_by_position(torch.empty(n, dtype=dtype, device=_dev()))]
    small = torch.cat([FR.expected_span(s, ln, dtype) for s, ln in zip(starts.tolist(), lens.tolist())])
    small_offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    yield {"tokens": hold[0], "offs": offs, "idx": idx, "small": small, "small_offs": small_offs}
    hold.clear()
    torch.cuda.empty_cache()


def _equal(got, ref, what):
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: output {k}"
        assert torch.equal(a.cpu(), b.cpu()), f"{what}: output {k} differs"


@pytest.mark.parametrize("pad_to", [0, 2047, 2049])
@pytest.mark.parametrize("max_blocks", [0, 1])
def test_gather_ragged_past_the_marks(corpus, max_blocks, pad_to):
    """``pad_to``: the batch is padded with empty sequences up to that many, on both sides of the LDS map's cap."""
    tokens, offs, idx = corpus["tokens"], corpus["offs"], corpus["idx"]
    assert _native.hip().RAGGED_MAP_CAP == 2047
    if pad_to:  # empty sequences: doubled entries behind the corpus's offsets
        n0 = len(offs) - 1
        extra = pad_to - len(idx)
        offs = np.concatenate([offs, np.full(extra, offs[-1])])
        idx = np.concatenate([idx[:3], n0 + np.arange(extra), idx[3:]])
        assert len(idx) == pad_to
    total = int(corpus["small"].numel())
    buf = torch.full((total + 32,), SENTINEL, dtype=tokens.dtype, device=_dev())
    out, dofs = ops.gather_ragged(tokens, offs, idx, out=buf[16:16 + total], max_blocks=max_blocks)
    torch.cuda.synchronize()
    lens = offs[idx + 1] - offs[idx]
    assert dofs.cpu().tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert torch.equal(out.cpu(), corpus["small"]), "gathered tokens differ from the formula"
    assert bool((buf[:16] == SENTINEL).all()) and bool((buf[16 + total:] == SENTINEL).all())


@pytest.mark.parametrize("pdt", [torch.int32, torch.int64])
@pytest.mark.parametrize("seq_len", [8, 6, 516])
def test_pad_pack_tokens_indexed_past_the_marks(corpus, seq_len, pdt):
    """Pad mode (``src_start`` at the marks) and pack mode (``seg_src`` past the marks) of
    ``pad_pack_tokens_indexed`` with labels, against the CPU references on the formula's tokens. The sequences
    cross the marks at an odd offset, so token and label loads sit on both sides of each."""
    tokens, offs, idx = corpus["tokens"], corpus["offs"], corpus["idx"]
    small, small_offs = corpus["small"], corpus["small_offs"]
    pad = ops.ref_pad_tokens(small, torch.from_numpy(small_offs), seq_len, PAD_ID, pdt)
    pad = (*pad, ops.ref_token_labels(pad[0], pad[1], None, -100))
    _equal(ops.pad_tokens_indexed(tokens, offs, idx, seq_len, PAD_ID, pdt, labels=True), pad, f"pad S={seq_len}")
    rs, re_, so = ops.ref_pack_plan(small_offs, seq_len)
    fill = len(rs) + 3
    r = ops.ref_pack_tokens(small, rs, re_, so, seq_len, PAD_ID, pdt, fill_rows=fill)
    pack = (*r, torch.from_numpy(so.astype(np.int32)), ops.ref_token_labels(r[0], r[1], r[3], -100))
    _equal(ops.pack_tokens_indexed(tokens, offs, idx, seq_len, PAD_ID, pdt, fill_rows=fill, labels=True), pack,
           f"pack S={seq_len}")


# ------------------------------------------------- flat pad_pack_tokens kernel
GUARD_BYTES = 64
RUN_LENS = (700, 0, 1, 7, 8, 9, 3, 530)  # contiguous sequences of one flat-stream run; 700 and 530 exceed every S


def _widen(v: np.ndarray) -> np.ndarray:
    """Token values as the kernels deliver them: int32 as is, 16-bit ids zero-extended."""
    return v.astype(np.int64) & 0xFFFF if v.dtype == np.int16 else v.astype(np.int64)


def _runs(dtype, n_elems):
    """Starts of the runs: 5 tokens in front of each byte and element mark inside the corpus, and the corpus's end."""
    eb = torch.empty((), dtype=dtype).element_size()
    total = sum(RUN_LENS)
    marks = sorted({m // eb for m in FR.MARKS} | set(FR.MARKS))
    return [m - 5 for m in marks if m + total < n_elems] + [n_elems - total]


def _loop_pad(dtype, offsets, S, pdt):
    """Per-token loop: row i = the first S tokens of stream[offsets[i]:offsets[i + 1]]."""
    B = len(offsets) - 1
    ids = np.full((B, S), PAD_ID, dtype=np.int64)
    mask, pos, lab = np.zeros((B, S), np.uint8), np.zeros((B, S), np.int64), np.full((B, S), -100, np.int64)
    for i in range(B):
        n = min(int(offsets[i + 1] - offsets[i]), S)
        tok = _widen(FR.expected(np.uint64(offsets[i]) + np.arange(n, dtype=np.uint64), dtype))
        for p in range(n):
            ids[i, p], mask[i, p], pos[i, p] = tok[p], 1, p
            if p + 1 < n:
                lab[i, p] = tok[p + 1]
    return (torch.from_numpy(ids.astype(np.int32)), torch.from_numpy(mask), torch.from_numpy(pos).to(pdt),
            torch.from_numpy(lab))


def _plan(offsets, S):
    """A packing plan built here: every sequence cut into segments of at most S tokens, consecutive segments put
    into a row while they fit. Rows are spans [row_start, row_end) of the flat stream."""
    so = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        so += list(range(int(a), int(b), S))
    so.append(int(offsets[-1]))
    rs, re_ = [], []
    for a, b in zip(so[:-1], so[1:]):
        if rs and b - rs[-1] <= S and re_[-1] == a:
            re_[-1] = b
        else:
            rs.append(a)
            re_.append(b)
    return np.asarray(rs, np.int64), np.asarray(re_, np.int64), np.asarray(so, np.int64)


def _loop_pack(dtype, plan, S, pdt):
    rs, re_, so = plan
    R = len(rs)
    ids = np.full((R, S), PAD_ID, dtype=np.int64)
    mask, pos = np.zeros((R, S), np.uint8), np.zeros((R, S), np.int64)
    seg, lab = np.full((R, S), -1, np.int64), np.full((R, S), -100, np.int64)
    for r in range(R):
        n = int(re_[r] - rs[r])
        assert 0 < n <= S
        tok = _widen(FR.expected(np.uint64(rs[r]) + np.arange(n, dtype=np.uint64), dtype))
        for p in range(n):
            g = int(rs[r]) + p
            s = max(j for j in range(len(so) - 1) if so[j] <= g)
            ids[r, p], mask[r, p], pos[r, p], seg[r, p] = tok[p], 1, g - so[s], s
            if p + 1 < n and g + 1 < so[s + 1]:
                lab[r, p] = tok[p + 1]
    return (torch.from_numpy(ids.astype(np.int32)), torch.from_numpy(mask), torch.from_numpy(pos).to(pdt),
            torch.from_numpy(seg.astype(np.int32)), torch.from_numpy(so.astype(np.int32)), torch.from_numpy(lab))


def _flat_launch(tokens, S, pdt, offsets=None, plan=None):
    dev = tokens.device
    if plan is None:
        rows, n_seg, dev_plan = len(offsets) - 1, None, (None, None, None)
        offs = torch.from_numpy(offsets).to(dev)
    else:
        dev_plan = tuple(torch.from_numpy(a).to(dev) for a in plan)
        rows, n_seg, offs = len(plan[0]), len(plan[2]) - 1, None
    need = ops.token_output_bytes(rows, S, n_seg, pdt, True)
    full = torch.full((GUARD_BYTES + need + GUARD_BYTES,), 0x5A, dtype=torch.uint8, device=dev)
    ids, mask, pos, seg, cu, lab = ops.carve_token_outputs(full[GUARD_BYTES:GUARD_BYTES + need], rows, S, n_seg, pdt, True)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    _native.hip().pad_pack_tokens(
        tokens=tokens.data_ptr(), offsets=ptr(offs), row_start=ptr(dev_plan[0]), row_end=ptr(dev_plan[1]),
        seg_offsets=ptr(dev_plan[2]), n_seg=n_seg or 0, out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(),
        position_ids=pos.data_ptr(), pos_is_i64=pdt == torch.int64, segment_ids=ptr(seg), cu_seqlens_out=ptr(cu),
        rows=rows, seq_len=S, pad_id=PAD_ID, mode=0 if plan is None else 1,
        stream=torch.cuda.current_stream(dev).cuda_stream, tok16=tokens.dtype == torch.int16, labels=lab.data_ptr(),
        ignore_index=-100)
    torch.cuda.synchronize()
    host = full.cpu()
    assert bool((host[:GUARD_BYTES] == 0x5A).all()) and bool((host[GUARD_BYTES + need:] == 0x5A).all())
    return (ids, mask, pos, lab) if plan is None else (ids, mask, pos, seg, cu, lab)


@pytest.mark.parametrize("pdt", [torch.int32, torch.int64])
@pytest.mark.parametrize("seq_len", [8, 6, 516])
def test_flat_pad_pack_tokens_past_the_marks(corpus, seq_len, pdt):
    """The flat kernel reading the corpus as its stream: pad mode with ``offsets`` at the marks, pack mode with a
    plan whose ``row_start`` / ``seg_offsets`` lie past them, labels on, against per-token loops over the formula.
    The run starts 5 tokens in front of a mark, so the label load at p0 + 4 is the token in front of the mark for
    the lane at p0 = 0 and the one at it for the next lane. ``cu_seqlens`` is the int32 the kernel stores of a flat
    position (a batch's own stream stays below 2^31; here it is the low 32 bits)."""
    tokens = corpus["tokens"]
    dtype, n = tokens.dtype, tokens.numel()
    for start in _runs(dtype, n):
        offsets = (start + np.concatenate([[0], np.cumsum(RUN_LENS)])).astype(np.int64)
        assert offsets[-1] <= n
        eb = tokens.element_size()
        FR.assert_no_alias([int(start)], sum(RUN_LENS), dtype, None, eb)
        _equal(_flat_launch(tokens, seq_len, pdt, offsets=offsets), _loop_pad(dtype, offsets, seq_len, pdt),
               f"flat pad S={seq_len} at {start}")
        plan = _plan(offsets, seq_len)
        _equal(_flat_launch(tokens, seq_len, pdt, plan=plan), _loop_pack(dtype, plan, seq_len, pdt),
               f"flat pack S={seq_len} at {start}")


# ------------------------------- descriptor, stream table and stream plans on the corpora
def _dict_equal(got, ref, what):
    for k, v in ref.items():
        g = got[k]
        assert g.dtype == v.dtype and tuple(g.shape) == tuple(v.shape), f"{what}: {k}"
        assert torch.equal(g.cpu(), v), f"{what}: {k} differs"


@pytest.mark.parametrize("seq_len", [8, 516])
def test_device_planned_batches_past_the_marks(corpus, seq_len):
    """``token_batch_descriptor`` (then ``pack_plan_device``) planning the batch on the device from device offsets
    and a device index, emitted through ``pad_pack_tokens_indexed``: the same rows as the host-planned ops, and the
    counts."""
    tokens, small, so_ = corpus["tokens"], corpus["small"], corpus["small_offs"]
    offs = torch.from_numpy(corpus["offs"]).to(_dev())
    index = torch.from_numpy(corpus["idx"]).to(_dev())
    n, lens = len(so_) - 1, np.diff(so_)
    ids, mask, pos = ops.ref_pad_tokens(small, torch.from_numpy(so_), seq_len, PAD_ID, torch.int64)
    ref = {"input_ids": ids, "attention_mask": mask, "position_ids": pos,
           "labels": ops.ref_token_labels(ids, mask, None, -100),
           "counts": torch.tensor([n, 0, int(so_[-1]), int(min(lens.max(), seq_len))])}
    got = ops.pad_tokens_indexed_device(tokens, offs, index=index, seq_len=seq_len, pad_id=PAD_ID, labels=True)
    torch.cuda.synchronize()
    _dict_equal(got, ref, f"device pad S={seq_len}")
    rs, re_, so = ops.ref_pack_plan(so_, seq_len)
    R, M, n_seg = len(rs) + 2, len(so) + 1, len(so) - 1
    ids, mask, pos, seg = ops.ref_pack_tokens(small, rs, re_, so, seq_len, PAD_ID, torch.int64, fill_rows=R)
    cu = torch.full((M + 1,), int(so_[-1]), dtype=torch.int32)
    cu[:n_seg + 1] = torch.from_numpy(so.astype(np.int32))
    ref = {"input_ids": ids, "attention_mask": mask, "position_ids": pos, "segment_ids": seg, "cu_seqlens": cu,
           "labels": ops.ref_token_labels(ids, mask, seg, -100),
           "counts": torch.tensor([len(rs), n_seg, int(so_[-1]), int(np.diff(so).max())])}
    got = ops.pack_tokens_indexed_device(tokens, offs, index=index, seq_len=seq_len, pad_id=PAD_ID, max_rows=R,
                                         max_segs=M, labels=True)
    torch.cuda.synchronize()
    _dict_equal(got, ref, f"device pack S={seq_len}")


def _loop_stream(dtype, offs, stream_rows, S, M, pdt):
    """The token stream of the corpus in document order (stream position g = corpus element g), rows
    ``stream_rows``, token by token: a segment is a maximal run of one document inside one row."""
    T, R = int(offs[-1]), len(stream_rows)
    ids = np.full((R, S), PAD_ID, dtype=np.int64)
    mask, pos = np.zeros((R, S), np.uint8), np.zeros((R, S), np.int64)
    seg, lab = np.full((R, S), -1, np.int64), np.full((R, S), -100, np.int64)
    starts, n_tok, n_seg, longest = [], 0, 0, 0
    for k, rho in enumerate(stream_rows):
        g0 = int(rho) * S
        n = max(min(S, T - g0), 0)
        tok = _widen(FR.expected(np.uint64(g0) + np.arange(n, dtype=np.uint64), dtype))
        prev, run = -1, 0
        for p in range(n):
            d = int(np.searchsorted(offs, g0 + p, side="right")) - 1
            if d != prev:
                starts.append(k * S + p)
                n_seg, prev, run = n_seg + 1, d, 0
            ids[k, p], mask[k, p], pos[k, p], seg[k, p] = tok[p], 1, run, n_seg - 1
            if p and seg[k, p - 1] == seg[k, p]:
                lab[k, p - 1] = tok[p]
            run += 1
            longest = max(longest, run)
        n_tok += n
    cu = np.full(M + 1, n_tok, dtype=np.int64)
    cu[:n_seg] = starts
    return {"input_ids": torch.from_numpy(ids.astype(np.int32)), "attention_mask": torch.from_numpy(mask),
            "position_ids": torch.from_numpy(pos).to(pdt), "segment_ids": torch.from_numpy(seg.astype(np.int32)),
            "cu_seqlens": torch.from_numpy(cu.astype(np.int32)), "labels": torch.from_numpy(lab),
            "counts": torch.tensor([-(-n_tok // S), n_seg, n_tok, longest])}


@pytest.mark.parametrize("pdt", [torch.int32, torch.int64])
@pytest.mark.parametrize("seq_len", [8, 6, 516])
def test_stream_table_and_plans_past_the_marks(corpus, seq_len, pdt):
    """``token_stream_table`` of the corpus's offsets, ``token_stream_plan`` for the rows across each mark (so
    ``row_base * S`` lies just below it) and across the corpus's end, and ``token_stream_plan_rows`` selecting the
    rows on both sides of each mark, each emitted through ``pad_pack_tokens_indexed`` with labels."""
    tokens, offs_np = corpus["tokens"], corpus["offs"]
    S, n = seq_len, tokens.numel()
    offs = torch.from_numpy(offs_np).to(_dev())
    table = ops.token_stream_table(offs)
    assert table.cpu().numpy().tolist() == offs_np.tolist()  # document order: the table is the offsets
    eb = tokens.element_size()
    marks = [m for m in sorted({m // eb for m in FR.MARKS} | set(FR.MARKS)) if m + 4 * S < n]
    M = 3 * 4
    for row_base in [m // S - 1 for m in marks] + [n // S - 1]:
        ref = _loop_stream(tokens.dtype, offs_np, [row_base + r for r in range(3)], S, M, pdt)
        got = ops.stream_tokens_indexed_device(tokens, offs, table, row_base=row_base, rows=3, seq_len=S,
                                               pad_id=PAD_ID, max_segs=M, position_dtype=pdt, labels=True)
        torch.cuda.synchronize()
        _dict_equal(got, ref, f"stream plan S={S} row_base={row_base}")
    rho = sorted({m // S + k for m in marks for k in (-1, 0, 1)} | {0, n // S - 1})
    rho = [int(r) for r in np.random.default_rng(6).permutation(rho)]
    M = 4 * len(rho)
    ref = _loop_stream(tokens.dtype, offs_np, rho, S, M, pdt)
    got = ops.stream_tokens_indexed_device(tokens, offs, table, row_base=0, rows=len(rho), seq_len=S, pad_id=PAD_ID,
                                           max_segs=M, position_dtype=pdt, labels=True, stream_rows=n // S,
                                           row_index=torch.tensor(rho, dtype=torch.int64, device=_dev()))
    torch.cuda.synchronize()
    _dict_equal(got, ref, f"stream row plan S={S}")
