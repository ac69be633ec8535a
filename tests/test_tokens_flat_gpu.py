"""The flat pad/pack kernel (``pad_pack_tokens``) against the CPU references and against the indexed ops on the
same data, bitwise: a corpus read with ``idx = arange(n)`` is its own gathered stream. Every launch writes into a
sentinel-filled buffer with guard bytes on each side, so an element the kernel leaves unwritten, or a store outside
the outputs, fails."""

import functools

import numpy as np
import pytest
import torch

from ddl_amd import _native, ops

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A
PAD_ID = -3


@functools.lru_cache(maxsize=None)
def _stream(np_dtype, seq_len, n_short=0):
    """(tokens, offsets): about 40 sequences of 0 .. 2 * seq_len + 3 tokens -- empty ones, the lengths around a row
    and around two rows -- or ``n_short`` sequences of 1 .. 3 tokens. Ids span the whole dtype."""
    rng = np.random.default_rng(11)
    S = seq_len
    if n_short:
        lens = 1 + np.arange(n_short) % 3
    else:
        lens = np.concatenate([[0, 1, 3, 4, 5, S - 1, S, S + 1, 0, 2 * S, 2 * S + 3, 0],
                               rng.integers(0, 2 * S + 4, size=28)])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    info = np.iinfo(np_dtype)
    return rng.integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True), offs


@functools.lru_cache(maxsize=None)
def _reference(np_dtype, seq_len, pdt, n_short=0, fill=0):
    """(pad outputs, pack outputs + cu_seqlens, the plan) of the CPU references; computed once, never modified."""
    toks, offs = _stream(np_dtype, seq_len, n_short)
    flat = torch.from_numpy(toks)
    rs, re_, so = ops.ref_pack_plan(offs, seq_len)
    pad = ops.ref_pad_tokens(flat, torch.from_numpy(offs), seq_len, PAD_ID, pdt)
    pack = (*ops.ref_pack_tokens(flat, rs, re_, so, seq_len, PAD_ID, pdt, fill_rows=fill),
            torch.from_numpy(so.astype(np.int32)))
    return pad, pack, (rs, re_, so)


def _launch(tokens, seq_len, pdt, offsets=None, plan=None, fill=0):
    """``pad_pack_tokens`` (pad mode: device ``offsets``; pack mode: the host ``plan``) into outputs carved from a
    sentinel-filled, guarded buffer. Returns the outputs as the ops order them."""
    dev = tokens.device
    if plan is None:
        rows, n_seg, R = offsets.numel() - 1, None, offsets.numel() - 1
        rs = re_ = so = None
    else:
        rs, re_, so = (torch.from_numpy(a).to(dev) for a in plan)
        rows, n_seg = rs.numel(), so.numel() - 1
        R = max(rows, fill)
    need = ops.token_output_bytes(R, seq_len, n_seg, pdt)
    full = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    assert full.data_ptr() % 16 == 0
    ids, mask, pos, seg, cu = ops.carve_token_outputs(full[GUARD:GUARD + need], R, seq_len, n_seg, pdt)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    rc = _native.hip().pad_pack_tokens(
        tokens=tokens.data_ptr(), offsets=ptr(offsets), row_start=ptr(rs), row_end=ptr(re_), seg_offsets=ptr(so),
        n_seg=n_seg or 0, out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(), position_ids=pos.data_ptr(),
        pos_is_i64=pdt == torch.int64, segment_ids=ptr(seg), cu_seqlens_out=ptr(cu), rows=rows, seq_len=seq_len,
        pad_id=PAD_ID, mode=0 if plan is None else 1, stream=torch.cuda.current_stream(dev).cuda_stream,
        fill_rows=fill, tok16=tokens.dtype == torch.int16)
    assert not rc
    torch.cuda.synchronize()
    host = full.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + need:] == SENTINEL).all())
    return (ids, mask, pos) if plan is None else (ids, mask, pos, seg, cu)


def _equal(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


def _check(np_dtype, seq_len, pdt, n_short=0):
    toks, offs = _stream(np_dtype, seq_len, n_short)
    pad_ref, pack_ref, plan = _reference(np_dtype, seq_len, pdt, n_short)
    tokens, idx = torch.from_numpy(toks).cuda(), np.arange(len(offs) - 1)
    _equal(_launch(tokens, seq_len, pdt, offsets=torch.from_numpy(offs).cuda()), pad_ref)
    _equal(ops.pad_tokens_indexed(tokens, offs, idx, seq_len, PAD_ID, pdt), pad_ref)
    _equal(_launch(tokens, seq_len, pdt, plan=plan), pack_ref)
    _equal(ops.pack_tokens_indexed(tokens, offs, idx, seq_len, PAD_ID, pdt), pack_ref)
    return tokens, idx, pack_ref, plan


@pytest.mark.parametrize("pdt", [torch.int64, torch.int32])
@pytest.mark.parametrize("seq_len", [6, 512, 516])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_flat_kernel_matches_the_references_and_the_indexed_ops_bitwise(np_dtype, seq_len, pdt):
    """seq_len 6: the per-element store path, every longer sequence split into many segments; 512: exactly one
    chunk; 516: a second chunk with one live lane. Pad, pack, and pack with ``fill_rows`` above the packed rows,
    from the host plan and through ``pack_tokens_device`` (the plan's counts read on the device)."""
    toks, offs = _stream(np_dtype, seq_len)
    tokens, idx, pack_ref, plan = _check(np_dtype, seq_len, pdt)
    rows, n_seg = pack_ref[0].shape[0], pack_ref[4].numel() - 1
    fill = rows + 5
    fill_ref = _reference(np_dtype, seq_len, pdt, fill=fill)[1]
    assert fill_ref[0].shape[0] == fill and bool((fill_ref[3][rows:] == -1).all())
    _equal(_launch(tokens, seq_len, pdt, plan=plan, fill=fill), fill_ref)
    _equal(ops.pack_tokens_indexed(tokens, offs, idx, seq_len, PAD_ID, pdt, fill_rows=fill), fill_ref)
    r = ops.pack_tokens_device(tokens, torch.from_numpy(offs).cuda(), seq_len, PAD_ID, pdt, max_rows=fill)
    assert r["counts"].tolist() == [rows, n_seg]
    _equal([r["input_ids"], r["attention_mask"], r["position_ids"], r["segment_ids"], r["cu_seqlens"][:n_seg + 1]],
           fill_ref)


@pytest.mark.parametrize("n_seq", [1000, 1100])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_flat_kernel_on_both_sides_of_the_lds_cap(np_dtype, n_seq):
    """Sequences of 1 .. 3 tokens at seq_len 6: every sequence is one segment, so n_seg + 1 is 1001 (staged in
    LDS) and 1101 (past the 1024 entries: the global-memory search)."""
    pack_ref = _check(np_dtype, 6, torch.int64, n_short=n_seq)[2]
    n_seg = pack_ref[4].numel() - 1
    assert n_seg + 1 == n_seq + 1
    assert (n_seg + 1 > _native.hip().TOKEN_SEG_LDS_CAP) == (n_seq == 1100)
