"""The device ragged gather against its reference, and the zero-copy token loader against its own CPU twin."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import _native, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GB = 16
WANTED = [0, 1, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1000, 0, 5]
GUARD = 64


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


def _source(toks: np.ndarray, kind: str):
    if kind == "device":
        return torch.from_numpy(toks).cuda(), None
    cpu = torch.from_numpy(toks).pin_memory()  # pinned and device-mapped
    return ops.HostRows(cpu, _native.hip().host_device_pointer(cpu.data_ptr())), cpu


def _check_gather(src, toks, offs, idx, max_blocks):
    ref, ref_offs = ops.ref_gather_ragged(torch.from_numpy(toks), offs, idx)
    total = ref.numel()
    sentinel = 0x5A5A if toks.dtype == np.int16 else 0x5A5A5A5A
    full = torch.full((GUARD + total + GUARD,), sentinel, dtype=ref.dtype, device="cuda")
    out, dofs = ops.gather_ragged(src, offs, idx, out=full[GUARD:GUARD + total], max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert out.numel() == total and (total == 0 or out.data_ptr() == full[GUARD:].data_ptr())
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(dofs.cpu(), ref_offs)
    host = full.cpu()
    assert bool((host[:GUARD] == sentinel).all()) and bool((host[GUARD + total:] == sentinel).all())


@pytest.mark.parametrize("max_blocks", [0, 1, 4])
@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_gather_ragged_matches_the_reference_bitwise(np_dtype, kind, max_blocks):
    toks, offs, idx = _ragged_corpus(np_dtype)
    src, _keep = _source(toks, kind)
    _check_gather(src, toks, offs, idx, max_blocks)


@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_gather_ragged_large_n_long_sequences_and_empty_batches(np_dtype):
    """More sequences than the LDS cap of the tile map (the global-memory search), sequences of several tiles,
    a batch of empty sequences and n = 0."""
    cap = _native.hip().RAGGED_MAP_CAP
    rng = np.random.default_rng(9)
    n_src = 5000
    lens = np.arange(n_src) % 13
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    info = np.iinfo(np_dtype)
    toks = rng.integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True)
    src, _keep = _source(toks, "host")
    idx = rng.integers(0, n_src, size=cap + 1000)
    assert len(idx) > cap
    _check_gather(src, toks, offs, idx, 4)
    _check_gather(src, toks, offs, idx[:cap], 0)  # the largest n that is searched in LDS
    _check_gather(src, toks, offs, np.zeros(0, np.int64), 0)  # n = 0: no launch
    _check_gather(src, toks, offs, np.array([0, 13, 26]), 1)  # only empty sequences: no tile
    lens = np.array([3, 20000, 5, 8192, 4096])  # a tile is 16 KB of source
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = rng.integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True)
    for kind in ("host", "device"):
        src, _keep = _source(toks, kind)
        _check_gather(src, toks, offs, np.array([1, 3, 4, 1, 0]), 4)


# ------------------------------------------------------------------- loader
def _corpus(token_dtype):
    return SharedTokenSource.synthetic(f"ddl_amd_zctg_{np.random.randint(1 << 30)}", 200, 0, 300, seed=3,
                                       vocab=65536, token_dtype=token_dtype)


def _same(a: dict, b: dict) -> None:
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k
        else:
            assert a[k] == b[k], k


def _twin(corpus, n_epochs, seq_len, mode, rank=0, world=1, **kw):
    """Every batch of the CPU twin with the same settings (computed once per test)."""
    for k in ("depth", "max_blocks", "handoff"):
        kw.pop(k, None)
    dl = ddl_amd.ZeroCopyTokenLoader(corpus, GB, seq_len, mode, DDLEnv(rank=rank, world_size=world), seed=4,
                                     device="cpu", n_epochs=n_epochs, **kw)
    out = []
    for _ in range(n_epochs):
        out += list(dl)
    return out


@pytest.mark.parametrize("seq_len,mode,token_dtype,pack_order,token_rows,depth,max_blocks,rank,world", [
    (100, "pad", "int32", "in_order", "exact", 1, 1, 0, 1),
    (256, "pack", "uint16", "ffd", "exact", 3, 0, 1, 2),
    (100, "pack", "int32", "in_order", "fixed", 1, 0, 3, 4),
    (256, "pad", "uint16", "in_order", "exact", 3, 1, 0, 1),
    (100, "pack", "uint16", "ffd", "fixed", 3, 1, 1, 2),
    (256, "pack", "int32", "ffd", "exact", 1, 0, 0, 1),
])
def test_loader_equals_its_cpu_twin(seq_len, mode, token_dtype, pack_order, token_rows, depth, max_blocks, rank,
                                    world):
    corpus = _corpus(token_dtype)
    try:
        kw = dict(pack_order=pack_order, token_rows=token_rows)
        ref = _twin(corpus, 2, seq_len, mode, rank, world, **kw)
        dl = ddl_amd.ZeroCopyTokenLoader(corpus, GB, seq_len, mode, DDLEnv(rank=rank, world_size=world), seed=4,
                                         n_epochs=2, depth=depth, max_blocks=max_blocks, **kw)
        got = []
        for _ in range(2):
            for b in dl:
                assert b["input_ids"].is_cuda
                got.append({k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in b.items()})
        assert len(got) == len(ref) == 24
        for a, b in zip(got, ref):
            _same(a, b)
        st = dl.stats()
        assert st["batches"] == 24 and st["max_blocks"] == max_blocks and st["handoff"] == "host"
        dl.close()
    finally:
        corpus.close()


@pytest.mark.parametrize("mode", ["pad", "pack"])
def test_held_batches_survive_the_rings(mode):
    """depth = 1: two device windows and three header slots. Every batch of an epoch (12, more than any ring)
    is kept, not cloned, and compared at the end -- cu_seqlens included: it is memory of its own."""
    corpus = _corpus("uint16")
    try:
        ref = _twin(corpus, 1, 100, mode)
        dl = ddl_amd.ZeroCopyTokenLoader(corpus, GB, 100, mode, seed=4, n_epochs=1, depth=1)
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
        dl = ddl_amd.ZeroCopyTokenLoader(corpus, GB, 256, "pack", seed=4, n_epochs=1, depth=3, handoff=handoff,
                                         max_blocks=8)
        outs = []
        for g, b in enumerate(dl):
            if g % 4 == 0:
                torch.cuda._sleep(2_000_000)  # the consumer's stream is busy; later gathers finish first
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


def test_two_loaders_share_one_registration():
    """Train + eval over one corpus: the second loader does not register the mapping again, and closing the
    first leaves it registered for the second."""
    from ddl_amd import zerocopy

    corpus = _corpus("int32")
    try:
        ref = _twin(corpus, 1, 100, "pack")
        a = ddl_amd.ZeroCopyTokenLoader(corpus, GB, 100, "pack", seed=4, n_epochs=1)
        b = ddl_amd.ZeroCopyTokenLoader(corpus, GB, 100, "pack", seed=4, n_epochs=1)
        assert a._reg_base == b._reg_base and zerocopy._SHARED_REGS[a._reg_base][1:] == [2, True]
        ita, itb = iter(a), iter(b)
        for g in range(3):
            _same(next(ita), ref[g])
            _same(next(itb), ref[g])
        base = a._reg_base
        a.close()
        assert zerocopy._SHARED_REGS[base][1] == 1 and _native.hip().pointer_is_host_registered(base)
        for g in range(3, 12):
            _same(next(itb), ref[g])
        b.close()
        assert base not in zerocopy._SHARED_REGS
    finally:
        corpus.close()
