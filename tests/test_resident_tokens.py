"""HBM-resident token loader on the CPU (the same planning with the host ragged gather and the host collate),
the indexed pad/pack ops on CPU tensors, and the host check of the kernel's index arithmetic."""

import shutil

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check

GB = 16


@pytest.fixture(params=["int32", "uint16"])
def corpus(request):
    """Lengths 0..300: empty sequences, and sequences longer than either seq_len."""
    src = SharedTokenSource.synthetic(f"ddl_amd_rt_{np.random.randint(1 << 30)}", 200, 0, 300, seed=3,
                                      vocab=65536, token_dtype=request.param)
    yield src
    src.close()


def _same(a: dict, b: dict) -> None:
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k
        else:
            assert a[k] == b[k], k


def _loader(cls, corpus, seq_len=100, mode="pack", rank=0, world=1, **kw):
    kw.setdefault("seed", 4)
    return cls(corpus, GB, seq_len, mode, DDLEnv(rank=rank, world_size=world), device="cpu", **kw)


def _resident(corpus, *a, **kw):
    return _loader(ddl_amd.ResidentTokenLoader, corpus, *a, **kw)


def _zerocopy(corpus, *a, **kw):
    return _loader(ddl_amd.ZeroCopyTokenLoader, corpus, *a, **kw)


@pytest.mark.parametrize("token_rows", ["exact", "fixed"])
@pytest.mark.parametrize("mode,pack_order", [("pad", "in_order"), ("pack", "in_order"), ("pack", "ffd")])
@pytest.mark.parametrize("seq_len", [100, 256])
def test_batches_equal_the_zerocopy_loader(corpus, seq_len, mode, pack_order, token_rows):
    kw = dict(pack_order=pack_order, token_rows=token_rows)
    rt, zc = _resident(corpus, seq_len, mode, **kw), _zerocopy(corpus, seq_len, mode, **kw)
    assert len(rt) == len(zc) == 12
    for _ in range(2):  # two epochs
        got, ref = list(rt), list(zc)
        assert len(got) == len(ref) == 12
        for a, b in zip(got, ref):
            _same(a, b)
    st = rt.stats()
    assert set(st) == {"batches", "source_bytes", "load_s", "load_gbps", "handoff", "host_waits", "replica_shared"}
    assert st["batches"] == 24 and st["source_bytes"] == corpus.tokens.n * corpus.token_bytes
    assert st["handoff"] == "device" and st["replica_shared"] is False
    rt.close()
    rt.close()  # a second close is harmless
    zc.close()


@pytest.mark.parametrize("mode", ["pad", "pack"])
def test_world_size_invariance(corpus, mode):
    """W = 1, 2, 4, 8: every global batch holds the same multiset of sequences (their real tokens, in rank
    order, are the W = 1 batch's)."""
    def real(b):
        return b["input_ids"][b["attention_mask"].bool()]

    one = [real(b) for b in _resident(corpus, 100, mode, n_epochs=1)]
    for world in (1, 2, 4, 8):
        ranks = [[real(b) for b in _resident(corpus, 100, mode, r, world, n_epochs=1)] for r in range(world)]
        assert all(len(r) == len(one) == 12 for r in ranks)
        for g in range(len(one)):
            assert torch.equal(torch.cat([ranks[r][g] for r in range(world)]), one[g]), (world, g)


def test_resume_from_a_zerocopy_state_and_back_and_across_world_sizes(corpus):
    full = list(_zerocopy(corpus, 100, "pack", n_epochs=1))
    zc = _zerocopy(corpus, 100, "pack", n_epochs=1)
    it = iter(zc)
    for _ in range(3):
        next(it)
    sd = zc.state_dict()
    assert sd["kind"] == "indexed" and sd["global_batch_cursor"] == 3
    rt = _resident(corpus, 100, "pack", n_epochs=1, resume_state=sd)  # zero-copy state -> resident loader
    it = iter(rt)
    for g in (3, 4, 5):
        _same(next(it), full[g])
    back = rt.state_dict()
    assert back["kind"] == "indexed" and back["global_batch_cursor"] == 6
    rest = list(_zerocopy(corpus, 100, "pack", n_epochs=1, resume_state=back))  # and back
    assert len(rest) == 6
    for a, b in zip(rest, full[6:]):
        _same(a, b)
    # a checkpoint taken at W = 2 resumes at W = 4: rank 1 of 4 continues with its own slice of batch 3, 4, ...
    two = _resident(corpus, 100, "pack", 0, 2, n_epochs=1)
    it = iter(two)
    for _ in range(3):
        next(it)
    sd2 = two.state_dict()
    assert sd2["world_size"] == 2
    got = list(_resident(corpus, 100, "pack", 1, 4, n_epochs=1, resume_state=sd2))
    ref = list(_zerocopy(corpus, 100, "pack", 1, 4, n_epochs=1))[3:]
    assert len(got) == len(ref) == 9
    for a, b in zip(got, ref):
        _same(a, b)


@pytest.mark.parametrize("position_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("seq_len", [6, 100])
def test_indexed_ops_on_cpu_tensors_equal_the_composed_references(corpus, seq_len, position_dtype):
    toks = corpus.tokens.tensor().view(-1)
    offs = corpus.offsets.tensor().view(-1)
    for idx in ([5, 0, 199, 5, 17, 42], [], [0]):
        idx = np.asarray(idx, dtype=np.int64)
        flat, dofs = ops.ref_gather_ragged(toks, offs, idx)
        got = ops.pad_tokens_indexed(toks, offs, idx, seq_len, pad_id=9, position_dtype=position_dtype)
        ref = ops.ref_pad_tokens(flat, dofs, seq_len, 9, position_dtype)
        assert len(got) == len(ref) == 3
        for a, b in zip(got, ref):
            assert a.dtype == b.dtype and torch.equal(a, b)
        rs, re_, so = ops.ref_pack_plan(dofs.numpy(), seq_len)
        for fill in (0, len(rs) + 2):
            got = ops.pack_tokens_indexed(toks, offs, idx, seq_len, pad_id=9, position_dtype=position_dtype,
                                          fill_rows=fill)
            ref = (*ops.ref_pack_tokens(flat, rs, re_, so, seq_len, 9, position_dtype, fill_rows=fill),
                   torch.from_numpy(so.astype(np.int32)))
            assert len(got) == len(ref) == 5
            for a, b in zip(got, ref):
                assert a.dtype == b.dtype and torch.equal(a, b)
            assert got[0].shape[0] == max(len(rs), fill)
    with pytest.raises(IndexError):
        ops.pack_tokens_indexed(toks, offs, [200], seq_len)


def test_output_carving_is_aligned_and_disjoint():
    """The regions of one output allocation: 16-byte aligned starts, in collate_token_window's order, no overlap,
    for element counts that are no multiple of 4."""
    for rows, s, n_seg, pdt in ((3, 37, 5, torch.int64), (3, 37, None, torch.int32), (0, 16, 0, torch.int64),
                                (2, 512, 1, torch.int32)):
        need = ops.token_output_bytes(rows, s, n_seg, pdt)
        whole = torch.zeros(need, dtype=torch.uint8)
        ids, mask, pos, seg, cu = ops.carve_token_outputs(whole, rows, s, n_seg, pdt)
        regions = [t for t in (pos, cu, ids, seg, mask) if t is not None]
        assert ids.shape == mask.shape == pos.shape == (rows, s) and pos.dtype == pdt
        assert (seg is None) == (cu is None) == (n_seg is None)
        end = whole.data_ptr()
        for t in regions:
            if t.numel():
                assert (t.data_ptr() - whole.data_ptr()) % 16 == 0 and t.data_ptr() >= end
                end = t.data_ptr() + t.numel() * t.element_size()
        assert end <= whole.data_ptr() + need


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_indexed_pad_pack_arithmetic_under_asan_ubsan(tmp_path):
    """The kernel's per-lane loops (csrc/kernels/tokens_indexed.h), replayed on the host over exact-size heap
    buffers for the corpus, the descriptor and the outputs: a plain executable, nothing preloaded."""
    run_host_check(tmp_path, "tokens_indexed_check", "tokens indexed check ok")
