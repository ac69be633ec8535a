"""Zero-copy token loader on the CPU (the same code path with the host ragged gather and the host collate),
the reference of the ragged gather op, and the host check of the kernel's index arithmetic."""

import shutil

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource, TokenBatchProducer, expected_tokens
from ddl_amd.permutation import EpochOrder
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check

GB = 16


@pytest.fixture(params=["int32", "uint16"])
def corpus(request):
    """Lengths 0..300: empty sequences, and sequences longer than either seq_len."""
    src = SharedTokenSource.synthetic(f"ddl_amd_zct_{np.random.randint(1 << 30)}", 200, 0, 300, seed=3,
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


def _loader(corpus, seq_len=100, mode="pack", rank=0, world=1, **kw):
    kw.setdefault("seed", 4)
    return ddl_amd.ZeroCopyTokenLoader(corpus, GB, seq_len, mode, DDLEnv(rank=rank, world_size=world),
                                       device="cpu", **kw)


@pytest.mark.parametrize("mode,pack_order", [("pad", "in_order"), ("pack", "in_order"), ("pack", "ffd")])
@pytest.mark.parametrize("seq_len", [100, 256])
def test_batches_equal_the_producer_path(corpus, seq_len, mode, pack_order, monkeypatch):
    monkeypatch.setenv("DDL_DEVICE", "cpu")
    zc = _loader(corpus, seq_len, mode, pack_order=pack_order)
    with ddl_amd.start(n_producers=2) as (env, conn):
        prod = TokenBatchProducer(corpus, GB, seq_len, mode, pack_order=pack_order)
        dl = ddl_amd.DistributedDataLoader(prod, GB, conn, 2, env=env, auto_mark=True,
                                           output=ddl_amd.OutputSpec(collate="tokens"),
                                           order=ddl_amd.OrderSpec(mode="indexed", seed=4))
        assert len(dl) == len(zc) == EpochOrder(corpus.n, GB, 4).batches_per_epoch
        for _ in range(2):
            got = list(zc)
            ref = list(dl)
            assert len(got) == len(ref) == 12
            for a, b in zip(got, ref):
                _same(a, b)
    zc.close()


def test_fixed_rows_and_keys(corpus):
    zc = _loader(corpus, 100, "pack", token_rows="fixed")
    b = next(iter(zc))
    assert set(b) == {"input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "max_seqlen",
                      "n_tokens", "n_rows"}
    assert b["input_ids"].shape == (zc.layout.max_segments, 100) and b["n_rows"] <= zc.layout.max_segments
    assert set(next(iter(_loader(corpus, 100, "pad")))) == {"input_ids", "attention_mask", "position_ids", "n_tokens"}
    st = zc.stats()
    assert set(st) == {"batches", "source_bytes", "max_blocks", "handoff", "host_waits", "prefault_s"}
    assert st["batches"] == 1 and st["source_bytes"] == corpus.tokens.n * corpus.token_bytes


@pytest.mark.parametrize("mode", ["pad", "pack"])
def test_world_size_invariance(corpus, mode):
    """The ranks' real tokens, concatenated in rank order, are the W = 1 batch's, for every batch of an epoch."""
    def real(b):
        return b["input_ids"][b["attention_mask"].bool()]

    one = [real(b) for b in _loader(corpus, 100, mode, n_epochs=1)]
    order = EpochOrder(corpus.n, GB, 4)
    if mode == "pack":  # pack mode keeps every token: the W = 1 batch is the corpus's sequences in order
        for g, t in enumerate(one):
            assert np.array_equal(t.numpy(), np.concatenate(expected_tokens(corpus, order.indices(0, g))))
    for world in (1, 2, 4, 8):
        ranks = [[real(b) for b in _loader(corpus, 100, mode, r, world, n_epochs=1)] for r in range(world)]
        assert all(len(r) == len(one) == 12 for r in ranks)
        for g in range(len(one)):
            assert torch.equal(torch.cat([ranks[r][g] for r in range(world)]), one[g]), (world, g)


def test_resume_mid_epoch_and_across_world_sizes(corpus):
    full = list(_loader(corpus, 100, "pack", n_epochs=1))
    dl = _loader(corpus, 100, "pack", n_epochs=1)
    it = iter(dl)
    for _ in range(3):
        next(it)
    sd = dl.state_dict()
    assert sd["kind"] == "indexed" and sd["global_batch_cursor"] == 3
    rest = list(_loader(corpus, 100, "pack", n_epochs=1, resume_state=sd))
    assert len(rest) == len(full) - 3
    for a, b in zip(rest, full[3:]):
        _same(a, b)
    # a checkpoint taken at W = 2 resumes at W = 4: rank 1 of 4 continues with its own slice of batch 3, 4, ...
    two = _loader(corpus, 100, "pack", 0, 2, n_epochs=1)
    it = iter(two)
    for _ in range(3):
        next(it)
    sd2 = two.state_dict()
    assert sd2["world_size"] == 2
    got = list(_loader(corpus, 100, "pack", 1, 4, n_epochs=1, resume_state=sd2))
    ref = list(_loader(corpus, 100, "pack", 1, 4, n_epochs=1))[3:]
    assert len(got) == len(ref) == 9
    for a, b in zip(got, ref):
        _same(a, b)


def test_ref_gather_ragged(corpus):
    toks = corpus.tokens.tensor().view(-1)
    offs = corpus.offsets.tensor().view(-1)
    idx = np.array([5, 0, 199, 5, 17, 42], dtype=np.int64)
    out, dofs = ops.ref_gather_ragged(toks, offs, idx)
    exp = expected_tokens(corpus, idx)
    assert np.array_equal(ops.kernels.widen_tokens(out).numpy(), np.concatenate(exp))
    assert dofs.dtype == torch.int64 and dofs.tolist() == [0, *np.cumsum([len(x) for x in exp]).tolist()]
    out2, _ = ops.gather_ragged(toks, offs, idx)  # a CPU source dispatches to the reference
    assert torch.equal(out, out2)
    empty, z = ops.ref_gather_ragged(toks, offs, [])
    assert empty.numel() == 0 and z.tolist() == [0]
    with pytest.raises(IndexError):
        ops.ref_gather_ragged(toks, offs, [200])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_ragged_index_arithmetic_under_asan_ubsan(tmp_path):
    """The kernel's tile / unit / mask arithmetic (csrc/kernels/ragged_index.h), emulated tile by tile on the
    host over exact-size heap buffers: a plain executable, nothing preloaded."""
    run_host_check(tmp_path, "ragged_index_check", "ragged index check ok")
