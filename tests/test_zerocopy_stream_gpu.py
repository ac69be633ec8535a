"""``ZeroCopyTokenStreamLoader`` on the GPU against ``ResidentTokenStreamLoader``, batch by batch and key by key."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import _native, ops, zerocopy
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GB, S, N_DOCS = 8, 64, 200


def _corpus(token_dtype, max_len=300):
    return SharedTokenSource.synthetic(f"ddl_amd_zcsg_{np.random.randint(1 << 30)}", N_DOCS, 0, max_len, seed=3,
                                       vocab=65536, token_dtype=token_dtype)


def _same(a: dict, b: dict) -> None:
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _epochs(dl, n):
    out = []
    for _ in range(n):
        for b in dl:
            out.append({k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in b.items()})
    return out


def _mix():
    return ddl_amd.TokenMix([0, 80, N_DOCS], [1.5, 0.5])


@pytest.mark.parametrize("token_dtype,max_blocks,kw", [
    ("uint16", 0, {}),
    ("int32", 1, dict(shuffle_rows=True)),
    ("uint16", 2, dict(mix="mix")),
    ("int32", 0, dict(labels=True)),
    ("uint16", 1, dict(shuffle=False)),
    ("uint16", 0, dict(shuffle_rows=True, mix="mix", labels=True)),
])
def test_batches_equal_the_resident_loader_over_two_epochs(token_dtype, max_blocks, kw):
    corpus = _corpus(token_dtype)
    try:
        kw = {k: _mix() if v == "mix" else v for k, v in kw.items()}
        res = ddl_amd.ResidentTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=2, **kw)
        want = _epochs(res, 2)
        res.close()
        dl = ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=2, max_blocks=max_blocks, **kw)
        got = _epochs(dl, 2)
        assert len(got) == len(want) == 2 * dl.batches_per_epoch > 0
        for a, b in zip(got, want):
            assert a["input_ids"].is_cuda and bool(a["attention_mask"].all())
            _same(a, b)
        st = dl.stats()
        assert st["format"] == "stream" and st["max_blocks"] == max_blocks and st["handoff"] == "host"
        assert st["batches"] == len(got) and st["tables_built"] == 2 and st["source_bytes"] == dl.nbytes
        dl.close()
        dl.close()
    finally:
        corpus.close()


def test_ranks_of_two_give_the_batch_of_one_and_held_batches_survive_the_ring():
    corpus = _corpus("uint16")
    try:
        one = ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=1, depth=1)
        held = list(one)  # kept, not cloned: more batches than the ring has windows
        ranks = [_epochs(ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(rank=r, world_size=2), seed=4,
                                                           n_epochs=1), 1) for r in range(2)]
        torch.cuda.synchronize()
        assert len(held) == len(ranks[0]) == len(ranks[1]) > 3
        for g, b in enumerate(held):
            for k in ("input_ids", "position_ids", "attention_mask"):
                assert torch.equal(torch.cat([ranks[0][g][k], ranks[1][g][k]]), b[k]), (g, k)
        cpu = _epochs(ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=1, device="cpu"), 1)
        for a, b in zip(held, cpu):
            _same({k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in a.items()}, b)
        one.close()
    finally:
        corpus.close()


def test_a_state_saved_by_one_loader_resumes_in_the_other():
    corpus = _corpus("int32")
    try:
        full = _epochs(ddl_amd.ResidentTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=1), 1)
        zc = ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=1)
        it = iter(zc)
        for _ in range(3):
            next(it)
        sd = zc.state_dict()
        assert sd["kind"] == "token_stream" and sd["global_batch_cursor"] == 3
        res = ddl_amd.ResidentTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=1, resume_state=sd)
        _same(next(iter(res)), full[3])
        back = ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(rank=1, world_size=2), seed=4, n_epochs=1,
                                                 resume_state=res.state_dict())
        assert torch.equal(next(iter(back))["input_ids"], full[4]["input_ids"][GB // 2:])
        for x in (zc, res, back):
            x.close()
    finally:
        corpus.close()


def test_hbm_bytes_is_the_stated_sum_and_does_not_scale_with_the_tokens():
    small, large = _corpus("uint16"), _corpus("uint16", 600)
    try:
        assert large.offsets.tensor()[-1] > 1.8 * small.offsets.tensor()[-1]
        sizes = []
        for corpus in (small, large):
            dl = ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, depth=3, max_segments=96,
                                                   shuffle_rows=True, prefault=False)
            scratch = _native.hip().token_stream_table_scratch(N_DOCS)
            want = (8 * (2 * (N_DOCS + 1) + scratch) + 8 * (N_DOCS + 1)
                    + 4 * ops.stream_zerocopy_window_bytes(GB, S, 96, 2, True))
            st = dl.stats()
            assert st["hbm_bytes"] == dl.hbm_bytes == want and st["prefault_s"] == 0.0
            held = sum(t.numel() * t.element_size() for t in (*dl._tables, dl._scratch, dl._offsets_dev, *dl._windows))
            assert held == want  # and it is what the loader allocated
            sizes.append(want)
            dl.close()
        assert sizes[0] == sizes[1]
    finally:
        small.close()
        large.close()


def test_close_unregisters_and_a_shared_mapping_survives_another_loader():
    corpus = _corpus("uint16")
    try:
        hip = _native.hip()
        dl = ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=1)
        base = dl._reg_base
        assert zerocopy._SHARED_REGS[base][1:] == [1, True] and hip.pointer_is_host_registered(base)
        assert dl.stats()["prefault_s"] > 0
        other = ddl_amd.ZeroCopyTokenLoader(corpus, GB, S, "pack", seed=4, n_epochs=1)
        assert other._reg_base == base and zerocopy._SHARED_REGS[base][1] == 2
        first = next(iter(dl))["input_ids"].clone()
        dl.close()
        assert zerocopy._SHARED_REGS[base][1] == 1 and hip.pointer_is_host_registered(base)
        assert next(iter(other))["input_ids"].is_cuda  # the other loader still reads the mapping
        other.close()
        assert base not in zerocopy._SHARED_REGS and not hip.pointer_is_host_registered(base)
        again = ddl_amd.ZeroCopyTokenStreamLoader(corpus, GB, S, DDLEnv(), seed=4, n_epochs=1)
        assert torch.equal(next(iter(again))["input_ids"], first)
        again.close()
        assert base not in zerocopy._SHARED_REGS and not hip.pointer_is_host_registered(base)
    finally:
        corpus.close()
