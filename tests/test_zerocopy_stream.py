"""``ZeroCopyTokenStreamLoader`` on the CPU: its twin runs the definition, ``ops.ref_stream_tokens``; the constructor's
refusals and the checkpoint are the stream format's."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.token_stream import TokenStreamLoader
from ddl_amd.types import DDLEnv

GB, S, N_DOCS = 8, 64, 200
KEYS = ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens")


@pytest.fixture(scope="module")
def source():
    src = SharedTokenSource.synthetic(f"ddl_amd_zcs_{np.random.randint(1 << 30)}", N_DOCS, 0, 300, seed=3,
                                      vocab=65536, token_dtype="uint16")
    yield src
    src.close()


def _loader(source, rank=0, world=1, **kw):
    kw.setdefault("seed", 4)
    return ddl_amd.ZeroCopyTokenStreamLoader(source, GB, S, DDLEnv(rank=rank, world_size=world), device="cpu", **kw)


def test_cpu_twin_batches_are_the_definition(source):
    dl = _loader(source, labels=True, n_epochs=2)
    assert isinstance(dl, TokenStreamLoader) and dl.handoff == "host"
    toks, offs = source.tokens.tensor().view(-1), source.offsets.tensor().view(-1)
    T = int(offs[-1])
    assert len(dl) == T // S // GB
    for e in range(2):
        batches = list(dl)
        assert len(batches) == T // S // GB
        for g, b in enumerate(batches):
            ref = ops.ref_stream_tokens(toks, offs, perm=FeistelPermutation(N_DOCS, 4, e), row_base=g * GB, rows=GB,
                                        seq_len=S, max_segs=dl.max_segments, labels=True)
            assert list(b) == [*KEYS, "labels", "max_seqlen", "n_tokens", "n_rows", "n_seg"]
            for k in (*KEYS, "labels"):
                assert torch.equal(b[k], ref[k]), (e, g, k)
            assert int(b["n_rows"]) == GB and int(b["n_seg"]) == int(ref["counts"][1])
    st = dl.stats()
    assert st["format"] == "stream" and st["hbm_bytes"] == 0 and st["source_bytes"] == 2 * T
    assert st["max_blocks"] == dl.max_blocks and st["prefault_s"] == 0.0 and st["batches"] == 2 * (T // S // GB)
    dl.close()
    dl.close()


def test_cpu_twin_equals_the_resident_twin_with_every_option(source):
    mix = ddl_amd.TokenMix([0, 80, N_DOCS], [1.5, 0.5])
    for kw in (dict(shuffle_rows=True), dict(mix=mix), dict(shuffle=False), dict(shuffle_rows=True, mix=mix, labels=True)):
        a = _loader(source, 1, 2, n_epochs=1, **kw)
        b = ddl_amd.ResidentTokenStreamLoader(source, GB, S, DDLEnv(rank=1, world_size=2), device="cpu", seed=4,
                                              n_epochs=1, **kw)
        xa, xb = list(a), list(b)
        assert len(xa) == len(xb) > 0
        for p, q in zip(xa, xb):
            assert list(p) == list(q)
            for k in p:
                assert torch.equal(torch.as_tensor(p[k]), torch.as_tensor(q[k])), (kw, k)
        a.close()
        b.close()


def test_constructor_refusals(source):
    with pytest.raises(ValueError, match="divisible"):
        _loader(source, 0, 3)
    with pytest.raises(ValueError, match="fewer than one global batch"):
        ddl_amd.ZeroCopyTokenStreamLoader(source, 1 << 20, S, DDLEnv(), device="cpu")
    with pytest.raises(ValueError, match="overflow int32 cu_seqlens"):
        ddl_amd.ZeroCopyTokenStreamLoader(source, 1 << 20, 1 << 12, DDLEnv(), device="cpu")
    with pytest.raises(ValueError, match="handoff"):
        _loader(source, handoff="later")
    with pytest.raises(ValueError, match="max_blocks"):
        _loader(source, max_blocks=-1)
    indexed = ddl_amd.ZeroCopyTokenLoader(source, GB, S, "pack", DDLEnv(), device="cpu", seed=4)
    with pytest.raises(ValueError, match="token stream"):
        _loader(source, resume_state=indexed.state_dict())
    indexed.close()


def test_state_dict_round_trip_and_exchange_with_the_resident_loader(source):
    full = [b["input_ids"] for b in _loader(source, n_epochs=1)]
    dl = _loader(source, 0, 2, n_epochs=1)
    it = iter(dl)
    for _ in range(3):
        next(it)
    sd = dl.state_dict()
    assert sd["kind"] == "token_stream" and sd["global_batch_cursor"] == 3 and sd["world_size"] == 2
    back = _loader(source, n_epochs=1, resume_state=sd)
    assert back.state_dict() == dict(sd, world_size=1)
    assert torch.equal(next(iter(back))["input_ids"], full[3])
    resident = ddl_amd.ResidentTokenStreamLoader(source, GB, S, DDLEnv(), device="cpu", seed=4, n_epochs=1,
                                                 resume_state=sd)
    assert torch.equal(next(iter(resident))["input_ids"], full[3])
    live = _loader(source, n_epochs=1)
    live.load_state_dict(resident.state_dict())  # the resident loader handed out batch 3: the cursor is behind it
    assert torch.equal(next(iter(live))["input_ids"], full[4])
    with pytest.raises(ValueError, match="shuffle_rows"):
        _loader(source, shuffle_rows=True, resume_state=sd)
    for x in (dl, back, resident, live):
        x.close()
