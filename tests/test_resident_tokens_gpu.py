"""The indexed pad/pack kernel against the composed CPU reference (bitwise), and the HBM-resident token loader
against its own CPU twin."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import _native, corpus_replica, ops
from ddl_amd.exceptions import DDLError
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GB = 16
WANTED = [0, 1, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1000, 0, 5]
GUARD = 64
SENTINEL = 0x5A


def _ragged_corpus(np_dtype, wanted=WANTED):
    """(tokens, offsets, idx): the wanted sequences with fillers between them so that wanted sequence i starts
    at residue i % 8 (elements) -- every residue modulo 8; idx also holds a repeated index and the corpus's
    first and last sequence."""
    lens, idx, at = [6], [], 6
    for i, n in enumerate(wanted):
        fill = (i - at) % 8
        lens += [fill, n]
        idx.append(len(lens) - 1)
        at += fill + n
    lens.append(11)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert sorted({int(offs[i]) % 8 for i in idx}) == list(range(8))
    idx += [0, len(lens) - 1, idx[9], idx[12]]
    rng = np.random.default_rng(5)
    info = np.iinfo(np_dtype)
    toks = rng.integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True)
    return toks, offs, np.asarray(idx, dtype=np.int64)


def _reference(toks, offs, idx, seq_len, pad_id, pdt, fill):
    """(pad outputs, pack outputs) of the composed CPU reference: ref_gather_ragged, then ref_pad_tokens /
    ref_pack_plan + ref_pack_tokens."""
    flat, dofs = ops.ref_gather_ragged(torch.from_numpy(toks), offs, idx)
    pad = ops.ref_pad_tokens(flat, dofs, seq_len, pad_id, pdt)
    rs, re_, so = ops.ref_pack_plan(dofs.numpy(), seq_len)
    pack = (*ops.ref_pack_tokens(flat, rs, re_, so, seq_len, pad_id, pdt, fill_rows=fill),
            torch.from_numpy(so.astype(np.int32)))
    return pad, pack


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


def _check_ops(toks, offs, idx, seq_len, pdt=torch.int64, fill=0, pad_id=-3):
    """Both ops, with and without ``out=`` (a slice of a sentinel-filled buffer with guard bytes on each side),
    bitwise against the composed reference."""
    pad_ref, pack_ref = _reference(toks, offs, idx, seq_len, pad_id, pdt, fill)
    corpus = torch.from_numpy(toks).cuda()
    _equal(ops.pad_tokens_indexed(corpus, offs, idx, seq_len, pad_id, pdt), pad_ref)
    _equal(ops.pack_tokens_indexed(corpus, offs, idx, seq_len, pad_id, pdt, fill_rows=fill), pack_ref)
    need = ops.token_output_bytes(len(idx), seq_len, None, pdt)
    full, out = _guarded(need)
    got = ops.pad_tokens_indexed(corpus, offs, idx, seq_len, pad_id, pdt, out=out)
    torch.cuda.synchronize()
    _equal(got, pad_ref)
    _check_guards(full, need)
    need = ops.token_output_bytes(pack_ref[0].shape[0], seq_len, pack_ref[4].numel() - 1, pdt)
    full, out = _guarded(need)
    got = ops.pack_tokens_indexed(corpus, offs, idx, seq_len, pad_id, pdt, fill_rows=fill, out=out)
    torch.cuda.synchronize()
    _equal(got, pack_ref)
    assert out.data_ptr() <= got[4].data_ptr() < out.data_ptr() + need  # carved from the caller's buffer
    _check_guards(full, need)
    return pack_ref


@pytest.mark.parametrize("seq_len", [6, 256, 512, 516])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_indexed_ops_match_the_composed_reference_bitwise(np_dtype, seq_len):
    """seq_len 6: no multiple of 4 (the scalar store path), sequences split into many segments, pad truncation;
    512: exactly one chunk; 516: a second chunk with one live lane."""
    toks, offs, idx = _ragged_corpus(np_dtype)
    _check_ops(toks, offs, idx, seq_len)
    _check_ops(toks, offs, idx, seq_len, pdt=torch.int32)


@pytest.mark.parametrize("n_seq,seq_len,global_search", [(1100, 37, False), (1100, 6, True), (1200, 37, True)])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_plans_around_the_lds_cap_of_the_segment_search(np_dtype, n_seq, seq_len, global_search):
    """Sequences of lengths i % 13. 1100 of them at seq_len 37 are 1015 segments (the 85 empty ones have none):
    just under the cap, staged in LDS. At seq_len 6 (lengths 7..12 split in two) and with 1200 sequences the plan
    has more than 1023 segments: the global-memory search."""
    lens = np.arange(n_seq) % 13
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    info = np.iinfo(np_dtype)
    toks = np.random.default_rng(9).integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True)
    idx = (np.arange(n_seq) * 7) % n_seq
    pack_ref = _check_ops(toks, offs, idx, seq_len)
    n_seg = pack_ref[4].numel() - 1
    assert (n_seg + 1 > _native.hip().TOKEN_SEG_LDS_CAP) == global_search


@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_degenerate_batches(np_dtype):
    toks, offs, idx = _ragged_corpus(np_dtype)
    empty = np.array([idx[0], idx[13], idx[0]])  # only empty sequences: zero rows, cu_seqlens == [0]
    assert (offs[empty + 1] - offs[empty] == 0).all()
    pack_ref = _check_ops(toks, offs, empty, 16)
    assert pack_ref[0].shape == (0, 16) and pack_ref[4].tolist() == [0]
    pack_ref = _check_ops(toks, offs, np.zeros(0, np.int64), 16)  # n = 0
    assert pack_ref[0].shape == (0, 16) and pack_ref[4].tolist() == [0]
    _check_ops(toks, offs, empty, 16, fill=5)  # only padding rows
    rows = _check_ops(toks, offs, idx, 256)[0].shape[0]
    pack_ref = _check_ops(toks, offs, idx, 256, fill=rows + 7)  # fill_rows greater than the packed rows
    assert pack_ref[0].shape[0] == rows + 7 and bool((pack_ref[3][rows:] == -1).all())


def test_bad_out_buffers_are_refused():
    toks, offs, idx = _ragged_corpus(np.int32)
    corpus = torch.from_numpy(toks).cuda()
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.pack_tokens_indexed(corpus, offs, idx, 256, out=buf[:64])  # too small
    with pytest.raises(ValueError):
        ops.pack_tokens_indexed(corpus, offs, idx, 256, out=buf[4:])  # not 16-byte aligned


# ------------------------------------------------------------------- loader
def _corpus(token_dtype):
    return SharedTokenSource.synthetic(f"ddl_amd_rtg_{np.random.randint(1 << 30)}", 200, 0, 300, seed=3,
                                       vocab=65536, token_dtype=token_dtype)


def _same(a: dict, b: dict) -> None:
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


def _twin(corpus, n_epochs, seq_len, mode, rank=0, world=1, **kw):
    """Every batch of the CPU twin with the same settings (computed once per test)."""
    for k in ("depth", "handoff"):
        kw.pop(k, None)
    dl = ddl_amd.ResidentTokenLoader(corpus, GB, seq_len, mode, DDLEnv(rank=rank, world_size=world), seed=4,
                                     device="cpu", n_epochs=n_epochs, **kw)
    out = []
    for _ in range(n_epochs):
        out += list(dl)
    return out


@pytest.mark.parametrize("seq_len,mode,token_dtype,pack_order,token_rows,depth,rank,world", [
    (100, "pad", "int32", "in_order", "exact", 1, 0, 1),
    (256, "pack", "uint16", "ffd", "exact", 3, 1, 2),
    (100, "pack", "int32", "in_order", "fixed", 1, 3, 4),
    (256, "pad", "uint16", "in_order", "exact", 3, 0, 1),
    (100, "pack", "uint16", "ffd", "fixed", 3, 1, 2),
    (256, "pack", "int32", "ffd", "exact", 1, 0, 1),
])
def test_loader_equals_its_cpu_twin(seq_len, mode, token_dtype, pack_order, token_rows, depth, rank, world):
    corpus = _corpus(token_dtype)
    try:
        kw = dict(pack_order=pack_order, token_rows=token_rows)
        ref = _twin(corpus, 2, seq_len, mode, rank, world, **kw)
        dl = ddl_amd.ResidentTokenLoader(corpus, GB, seq_len, mode, DDLEnv(rank=rank, world_size=world), seed=4,
                                         n_epochs=2, depth=depth, chunk_bytes=4096, **kw)
        got = []
        for _ in range(2):
            for b in dl:
                assert b["input_ids"].is_cuda
                got.append({k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in b.items()})
        assert len(got) == len(ref) == 24
        for a, b in zip(got, ref):
            _same(a, b)
        st = dl.stats()
        assert set(st) == {"batches", "source_bytes", "load_s", "load_gbps", "handoff", "host_waits",
                           "replica_shared"}
        assert st["batches"] == 24 and st["handoff"] == "device" and st["replica_shared"] is False
        assert st["source_bytes"] == corpus.tokens.n * corpus.token_bytes and st["load_s"] > 0
        dl.close()
        dl.close()  # harmless
    finally:
        corpus.close()


@pytest.mark.parametrize("mode", ["pad", "pack"])
def test_held_batches_are_memory_of_their_own(mode):
    """depth = 1: two descriptor windows and three pinned slots. Every batch of an epoch (12, more than any
    ring) is kept, not cloned, and compared at the end."""
    corpus = _corpus("uint16")
    try:
        ref = _twin(corpus, 1, 100, mode)
        dl = ddl_amd.ResidentTokenLoader(corpus, GB, 100, mode, seed=4, n_epochs=1, depth=1)
        held = list(dl)
        assert len(held) == len(ref) == 12
        torch.cuda.synchronize()
        for a, b in zip(held, ref):
            _same(a, b)
        dl.close()
    finally:
        corpus.close()


@pytest.mark.parametrize("handoff", ["host", "device"])
def test_handoff_modes_deliver_the_same_bytes_behind_a_busy_stream(handoff):
    corpus = _corpus("int32")
    try:
        ref = _twin(corpus, 1, 256, "pack")
        dl = ddl_amd.ResidentTokenLoader(corpus, GB, 256, "pack", seed=4, n_epochs=1, depth=3, handoff=handoff)
        outs = []
        for g, b in enumerate(dl):
            if g % 4 == 0:
                torch.cuda._sleep(2_000_000)  # the consumer's stream is busy; later batches finish first
            outs.append({k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in b.items()})
        del b
        assert len(outs) == len(ref)
        for a, r in zip(outs, ref):
            _same(a, r)
        st = dl.stats()
        assert st["handoff"] == handoff and (st["host_waits"] == 0 or handoff == "host")
        dl.close()
    finally:
        corpus.close()


def test_two_loaders_share_one_replica():
    """Train + eval over one corpus on one device: one replica in HBM, freed when the last loader closes."""
    corpus = _corpus("int32")
    try:
        ref = _twin(corpus, 1, 100, "pack")
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        a = ddl_amd.ResidentTokenLoader(corpus, GB, 100, "pack", seed=4, n_epochs=1)
        b = ddl_amd.ResidentTokenLoader(corpus, GB, 100, "pack", seed=4, n_epochs=1)
        assert a.replica_ptr == b.replica_ptr and a.replica_ptr is not None
        assert a.stats()["replica_shared"] is False and b.stats()["replica_shared"] is True
        key = a._replica.key
        assert b._replica is a._replica and corpus_replica.REPLICAS[key].users == 2
        assert torch.cuda.memory_allocated() >= before + a.nbytes
        ita, itb = iter(a), iter(b)
        for g in range(3):
            _same(next(ita), ref[g])
            _same(next(itb), ref[g])
        del ita
        a.close()
        assert a.replica_ptr is None and corpus_replica.REPLICAS[key].users == 1
        for g in range(3, 12):
            _same(next(itb), ref[g])
        del itb
        b.close()
        assert key not in corpus_replica.REPLICAS
        assert torch.cuda.memory_allocated() <= before  # the replica (and every window) went back to the allocator
    finally:
        corpus.close()


def test_over_budget_corpus_is_refused_and_leaves_nothing_behind():
    from ddl_amd import zerocopy

    corpus = _corpus("uint16")
    try:
        nbytes = corpus.tokens.n * corpus.token_bytes
        with pytest.raises(DDLError) as err:
            ddl_amd.ResidentTokenLoader(corpus, GB, 100, "pack", seed=4, hbm_fraction=0.0)
        assert str(nbytes) in str(err.value) and "ZeroCopyTokenLoader" in str(err.value)
        assert not corpus_replica.REPLICAS and not zerocopy._SHARED_REGS
        ref = _twin(corpus, 1, 100, "pack")
        dl = ddl_amd.ResidentTokenLoader(corpus, GB, 100, "pack", seed=4, n_epochs=1)  # a normal construction works
        for a, b in zip(list(dl), ref):
            _same(a, b)
        dl.close()
        assert not corpus_replica.REPLICAS and not zerocopy._SHARED_REGS
    finally:
        corpus.close()
