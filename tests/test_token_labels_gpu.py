"""Next-token labels written by the pad/pack kernels: the flat and the indexed ops, the device-planned ops and the
loaders on the GPU, bitwise against ``ref_token_labels`` of the CPU reference batch; with labels on, every other
output is bitwise what labels off gives."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import _native, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A
PAD = -3


def _guarded(need):
    full = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert full.data_ptr() % 16 == 0
    return full, full[GUARD:GUARD + need]


def _check_guards(full, need):
    host = full.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + need:] == SENTINEL).all())


def _equal(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b)


def _corpus(S, np_dtype, seed=5):
    """(tokens, offsets, idx). The batch holds lengths 0, 1, S - 1, S, S + 1, 2 S + 3; behind a full row a 512-token
    sequence followed by a short one (where S allows: a segment whose last token is at position 511 of its row),
    and the same with 513 tokens (at 512); the corpus's last sequence, a repeat, and random lengths in [0, 3 S]."""
    rng = np.random.default_rng(seed)
    wanted = [0, 1, S - 1, S, S + 1, 2 * S + 3, 0, 4, 5, 8]
    if S > 513:
        wanted += [S, 512, S - 512, S, 513, S - 513]
    wanted += rng.integers(0, 3 * S + 1, size=6).tolist() + [7]
    lens, idx = [3], []
    for i, n in enumerate(wanted):  # a filler in front of each: the starts walk the residues modulo 8
        lens += [i % 8, n]
        idx.append(len(lens) - 1)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx += [idx[5], 0]
    info = np.iinfo(np_dtype)
    toks = rng.integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True)
    return toks, offs, np.asarray(idx, dtype=np.int64)


def _reference(toks, offs, idx, S, pdt, fill, ignore):
    """The CPU reference batch (composed references) with its labels appended: (flat stream, its offsets, pad
    outputs + labels, pack outputs + labels)."""
    flat, dofs = ops.ref_gather_ragged(torch.from_numpy(toks), offs, idx)
    pad = ops.ref_pad_tokens(flat, dofs, S, PAD, pdt)
    rs, re_, so = ops.ref_pack_plan(dofs.numpy(), S)
    pack = (*ops.ref_pack_tokens(flat, rs, re_, so, S, PAD, pdt, fill_rows=fill), torch.from_numpy(so.astype(np.int32)))
    return (flat, dofs, (*pad, ops.ref_token_labels(pad[0], pad[1], None, ignore)),
            (*pack, ops.ref_token_labels(pack[0], pack[1], pack[3], ignore)))


def _check_ops(toks, offs, idx, S, pdt=torch.int64, fill=0, ignore=-100):
    """The indexed ops (into a guarded ``out=``) and the flat ops, labels on, against the reference; labels off
    gives the same other outputs."""
    flat, dofs, pad_ref, pack_ref = _reference(toks, offs, idx, S, pdt, fill, ignore)
    kw = dict(labels=True, ignore_index=ignore)
    corpus = torch.from_numpy(toks).cuda()
    # indexed, pad
    need = ops.token_output_bytes(len(idx), S, None, pdt, labels=True)
    full, out = _guarded(need)
    got = ops.pad_tokens_indexed(corpus, offs, idx, S, PAD, pdt, out=out, **kw)
    torch.cuda.synchronize()
    _equal(got, pad_ref)
    _check_guards(full, need)
    _equal(ops.pad_tokens_indexed(corpus, offs, idx, S, PAD, pdt), pad_ref[:3])
    # indexed, pack
    R, n_seg = pack_ref[0].shape[0], pack_ref[4].numel() - 1
    need = ops.token_output_bytes(R, S, n_seg, pdt, labels=True)
    full, out = _guarded(need)
    got = ops.pack_tokens_indexed(corpus, offs, idx, S, PAD, pdt, fill_rows=fill, out=out, **kw)
    torch.cuda.synchronize()
    _equal(got, pack_ref)
    if got[5].numel():  # carved from the caller's buffer, 16-byte aligned
        assert out.data_ptr() <= got[5].data_ptr() < out.data_ptr() + need and got[5].data_ptr() % 16 == 0
    _check_guards(full, need)
    _equal(ops.pack_tokens_indexed(corpus, offs, idx, S, PAD, pdt, fill_rows=fill), pack_ref[:5])
    # flat: the gathered stream on the device
    flat_d = flat.cuda()
    _equal(ops.pad_tokens(flat_d, dofs.cuda(), S, PAD, pdt, **kw), pad_ref)
    _equal(ops.pad_tokens(flat_d, dofs.cuda(), S, PAD, pdt), pad_ref[:3])
    if fill == 0:
        _equal(ops.pack_tokens(flat_d, dofs, S, PAD, pdt, **kw), pack_ref)  # the host plan
        _equal(ops.pack_tokens(flat_d, dofs, S, PAD, pdt), pack_ref[:5])
        _equal(ops.pack_tokens(flat_d, dofs.cuda(), S, PAD, pdt, **kw), pack_ref)  # the plan built on the device
    else:  # padding rows of the flat kernel: the device plan's static row count
        r = ops.pack_tokens_device(flat_d, dofs.cuda(), S, PAD, pdt, max_rows=R, **kw)
        _equal([r[k] for k in ("input_ids", "attention_mask", "position_ids", "segment_ids", "labels")],
               [pack_ref[i] for i in (0, 1, 2, 3, 5)])
    return pack_ref


@pytest.mark.parametrize("S", [16, 37, 520, 515])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_ops_write_the_reference_labels(np_dtype, S):
    """S = 16 / 520: the vector store path, 37 / 515: the scalar one; 520 and 515 have a second 512-position
    chunk. int64 and int32 position ids, ignore_index -100 and -7, fill_rows greater than the packed rows."""
    toks, offs, idx = _corpus(S, np_dtype)
    pack_ref = _check_ops(toks, offs, idx, S)
    _check_ops(toks, offs, idx, S, pdt=torch.int32, ignore=-7)
    rows = pack_ref[0].shape[0]
    pack_ref = _check_ops(toks, offs, idx, S, fill=rows + 3, ignore=-7)
    assert pack_ref[0].shape[0] == rows + 3 and bool((pack_ref[5][rows:] == -7).all())
    if S > 513:  # the segment ends the corpus was built for: last tokens at positions 511 and 512 of a row
        seg, lab = pack_ref[3], pack_ref[5]
        ends = {int(p) for r in range(rows) for p in (seg[r, 1:] != seg[r, :-1]).nonzero().flatten()}
        assert {511, 512} <= ends
        assert all(bool((lab[:, p] == -7).any()) for p in (511, 512))


@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_labels_with_the_segment_search_in_global_memory(np_dtype):
    """1100 sequences of 1-3 tokens at S = 16: n_seg + 1 > the LDS cap."""
    lens = 1 + np.arange(1100) % 3
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    info = np.iinfo(np_dtype)
    toks = np.random.default_rng(9).integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True)
    pack_ref = _check_ops(toks, offs, (np.arange(1100) * 7) % 1100, 16)
    assert pack_ref[4].numel() > _native.hip().TOKEN_SEG_LDS_CAP
    assert bool((pack_ref[5][0, :3] != -100).sum() >= 1)


@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_degenerate_batches(np_dtype):
    toks, offs, idx = _corpus(16, np_dtype)
    empty = np.array([idx[0], idx[6], idx[0]])  # only empty sequences
    assert (offs[empty + 1] - offs[empty] == 0).all()
    assert _check_ops(toks, offs, empty, 16)[5].shape == (0, 16)
    pack_ref = _check_ops(toks, offs, empty, 16, fill=5, ignore=-7)  # only padding rows
    assert pack_ref[5].shape == (5, 16) and bool((pack_ref[5] == -7).all())
    assert _check_ops(toks, offs, np.zeros(0, np.int64), 16)[5].shape == (0, 16)  # n = 0


def test_misaligned_labels_are_refused_on_the_vector_path():
    """The argument guards: 16-byte stores need a 16-byte aligned labels pointer (S a multiple of 4)."""
    h = _native.hip()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    offs = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    toks = torch.arange(4, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    kw = dict(row_start=0, row_end=0, seg_offsets=0, n_seg=0, out_tokens=p, attn_mask=p + 256, position_ids=p + 512,
              pos_is_i64=True, segment_ids=0, cu_seqlens_out=0, rows=1, seq_len=8, pad_id=0, mode=0,
              stream=torch.cuda.current_stream().cuda_stream, labels=p + 1024 + 8)
    with pytest.raises(Exception):
        h.pad_pack_tokens(tokens=toks.data_ptr(), offsets=offs.data_ptr(), **kw)
    src = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(Exception):
        h.pad_pack_tokens_indexed(corpus=toks.data_ptr(), corpus_elems=4, src_start=src.data_ptr(), seg_src=0,
                                  offsets=offs.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert not buf.any()  # nothing was launched


# ------------------------------------------------------------- device-planned ops
@pytest.mark.parametrize("S", [16, 37, 520, 515])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_device_planned_ops(np_dtype, S):
    """Through ``index=``, ``perm=`` and the identity, pad and pack, into a guarded ``out=``; an overflowing plan
    (``max_rows`` too small) gives labels that are all ``ignore_index``."""
    toks, offs, idx = _corpus(S, np_dtype)
    n_corpus = len(offs) - 1
    c_h, o_h = torch.from_numpy(toks), torch.from_numpy(offs)
    c_d, o_d = c_h.cuda(), o_h.cuda()
    perm = FeistelPermutation(n_corpus, seed=11, epoch=2)
    index = torch.from_numpy(idx)
    for ignore, pdt, sel_h, sel_d in (
            (-100, torch.int64, dict(index=index), dict(index=index.cuda())),
            (-7, torch.int32, dict(perm=perm, base=3, count=n_corpus - 5), dict(perm=perm, base=3, count=n_corpus - 5)),
            (-7, torch.int64, dict(base=2, count=n_corpus - 2), dict(base=2, count=n_corpus - 2))):
        n = len(idx) if "index" in sel_h else sel_h["count"]
        kw = dict(seq_len=S, pad_id=PAD, position_dtype=pdt)
        ref = ops.pad_tokens_indexed_device(c_h, o_h, **sel_h, **kw, labels=True, ignore_index=ignore)
        assert torch.equal(ref["labels"], ops.ref_token_labels(ref["input_ids"], ref["attention_mask"], None, ignore))
        need = ops.device_plan_bytes(n) + ops.device_batch_bytes(n, S, None, pdt, labels=True)
        full, out = _guarded(need)
        got = ops.pad_tokens_indexed_device(c_d, o_d, **sel_d, **kw, out=out, labels=True, ignore_index=ignore)
        off = ops.pad_tokens_indexed_device(c_d, o_d, **sel_d, **kw)
        torch.cuda.synchronize()
        _check_guards(full, need)
        assert set(got) == set(ref) == set(off) | {"labels"}
        for k in ref:
            assert got[k].dtype == ref[k].dtype and torch.equal(got[k].cpu(), ref[k]), k
            assert k == "labels" or torch.equal(off[k], got[k]), k
        ref = ops.pack_tokens_indexed_device(c_h, o_h, **sel_h, **kw, labels=True, ignore_index=ignore)
        assert torch.equal(ref["labels"], ops.ref_token_labels(ref["input_ids"], ref["attention_mask"],
                                                               ref["segment_ids"], ignore))
        R, M = ref["input_ids"].shape[0], ref["cu_seqlens"].numel() - 1
        need = ops.device_plan_bytes(n, M, R) + ops.device_batch_bytes(R, S, M, pdt, labels=True)
        full, out = _guarded(need)
        got = ops.pack_tokens_indexed_device(c_d, o_d, **sel_d, **kw, out=out, labels=True, ignore_index=ignore)
        off = ops.pack_tokens_indexed_device(c_d, o_d, **sel_d, **kw)
        torch.cuda.synchronize()
        _check_guards(full, need)
        assert set(got) == set(ref) == set(off) | {"labels"}
        for k in ref:
            assert got[k].dtype == ref[k].dtype and torch.equal(got[k].cpu(), ref[k]), k
            assert k == "labels" or torch.equal(off[k], got[k]), k
        got = ops.pack_tokens_indexed_device(c_d, o_d, **sel_d, **kw, max_rows=2, labels=True, ignore_index=ignore)
        assert int(got["counts"][0]) == -1 and got["labels"].shape == (2, S) and bool((got["labels"] == ignore).all())
        assert not bool(got["attention_mask"].any())


# ------------------------------------------------------------------------ loaders
def _source(S, token_dtype):
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 3 * S + 1, size=60)
    lens[:7] = [0, 1, S - 1, S, S + 1, 2 * S + 3, 0]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = rng.integers(0, 60000, size=int(offs[-1]), dtype=np.int32)
    return SharedTokenSource.create(f"ddl_amd_tlg_{np.random.randint(1 << 30)}", toks, offs, token_dtype)


def _make(cls, src, S, mode, device=None, **kw):
    return cls(src, 12, S, mode, DDLEnv(rank=0, world_size=1), seed=4, device=device, n_epochs=2, **kw)


TENSORS = ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "labels")


MODES = [("pad", "in_order", "exact"), ("pack", "in_order", "fixed"), ("pack", "ffd", "exact")]
LOADERS = [(w, *m) for w in ("resident", "resident-device", "zero-copy") for m in MODES
           if not (w == "resident-device" and m[1] == "ffd")]  # plan="device" builds in-order plans only


@pytest.mark.parametrize("S,token_dtype", [(37, "uint16"), (520, "int32")])
@pytest.mark.parametrize("which,mode,pack_order,token_rows", LOADERS)
def test_loaders_deliver_the_cpu_twins_labels(which, mode, pack_order, token_rows, S, token_dtype):
    """Two epochs; every batch is held, not cloned, to the end (more than depth + 2 later steps), then compared
    with the CPU twin's: labels included, and equal to the reference of the batch's own outputs."""
    cls = ddl_amd.ZeroCopyTokenLoader if which == "zero-copy" else ddl_amd.ResidentTokenLoader
    kw = dict(pack_order=pack_order, token_rows=token_rows, labels=True, ignore_index=-7)
    if which == "resident-device":
        kw["plan"] = "device"
    src = _source(S, token_dtype)
    try:
        twin = _make(cls, src, S, mode, device="cpu", **kw)
        dl = _make(cls, src, S, mode, depth=1, **kw)
        ref = list(twin) + list(twin)
        held = list(dl) + list(dl)
        torch.cuda.synchronize()
        assert len(held) == len(ref) == 10
        for a, b in zip(held, ref):
            assert a.keys() == b.keys() and "labels" in a
            for k in a:
                if isinstance(a[k], torch.Tensor):
                    assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k]), k
                else:
                    assert a[k] == b[k], k
            assert a["labels"].is_cuda and a["labels"].dtype == torch.int64
            assert torch.equal(a["labels"], ops.ref_token_labels(a["input_ids"], a["attention_mask"],
                                                                 a.get("segment_ids"), -7))
            if which != "zero-copy" or mode == "pack":  # carved from the batch's one allocation
                assert a["labels"].untyped_storage().data_ptr() == a["input_ids"].untyped_storage().data_ptr()
        dl.close()
        twin.close()
    finally:
        src.close()
