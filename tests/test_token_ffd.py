"""The device first-fit-decreasing order on the CPU: ``ops.ref_ffd_index`` (the definition of the
``token_ffd_order`` kernel) against ``ffd_if_it_wins`` applied by hand, the ops' reference paths,
``ResidentTokenLoader(plan="device", pack_order="ffd_device")`` against the host FFD plan, ``max_rows``, and the
host check of the kernel's index arithmetic."""

import shutil

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource, ffd_if_it_wins, ffd_order_py, in_order_rows_py
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check
from tests.test_resident_tokens_plan import same_as_host_plan

GB = 16


@pytest.fixture(params=["int32", "uint16"])
def corpus(request):
    """Lengths 0..300: empty sequences, and sequences longer than either seq_len."""
    src = SharedTokenSource.synthetic(f"ddl_amd_ffd_{np.random.randint(1 << 30)}", 200, 0, 300, seed=3,
                                      vocab=65536, token_dtype=request.param)
    yield src
    src.close()


def _loader(corpus, seq_len=100, rank=0, world=1, **kw):
    kw.setdefault("seed", 4)
    return ddl_amd.ResidentTokenLoader(corpus, GB, seq_len, kw.pop("mode", "pack"),
                                       DDLEnv(rank=rank, world_size=world), device="cpu", **kw)


def _host_ffd(corpus, *a, **kw):
    return _loader(corpus, *a, plan="host", pack_order="ffd", token_rows="fixed", **kw)


def _ffd_device(corpus, *a, **kw):
    return _loader(corpus, *a, plan="device", pack_order="ffd_device", **kw)


def test_ref_ffd_index_is_ffd_if_it_wins():
    rng = np.random.default_rng(0)
    seen = set()
    for trial in range(60):
        S = int(rng.choice([8, 37, 100]))
        n_corpus = int(rng.integers(1, 80))
        lens = rng.integers(0, 3 * S, n_corpus)
        if trial % 3 == 0:
            lens = np.full(n_corpus, S // 2)  # in-order pairs: FFD cannot win
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        q = rng.integers(0, n_corpus, int(rng.integers(0, 60))).astype(np.int64)
        idx, ffd_rows, in_order, used = ops.ref_ffd_index(torch.from_numpy(offs), len(q), torch.from_numpy(q),
                                                          seq_len=S)
        sel = lens[q]
        order = ffd_if_it_wins(sel, S)  # the native rule of every host path
        assert used == (order is not None)
        assert idx.dtype == torch.int64 and idx.tolist() == (q if order is None else q[order]).tolist()
        assert ffd_rows == ffd_order_py(sel, S)[1] and in_order == in_order_rows_py(sel, S)
        assert min(ffd_rows, in_order) == (ffd_rows if used else in_order)
        seen.add(used)
    assert seen == {0, 1}
    # the other selectors, and an index outside the corpus (an empty sequence)
    offs = torch.tensor([0, 5, 5, 12, 20, 23])
    perm = FeistelPermutation(5, seed=1, epoch=0)
    want = perm(np.arange(1, 5))
    idx, *_ = ops.ref_ffd_index(offs, 4, perm=perm, base=1, seq_len=8)
    assert sorted(idx.tolist()) == sorted(want.tolist())
    idx, ffd_rows, in_order, used = ops.ref_ffd_index(offs, 3, base=2, seq_len=8)
    assert sorted(idx.tolist()) == [2, 3, 4] and ffd_rows <= in_order + (1 - used) * ffd_rows
    idx, ffd_rows, in_order, used = ops.ref_ffd_index(offs, 4, torch.tensor([2, 99, 3, -1]), seq_len=8)
    assert (ffd_rows, in_order, used) == (2, 2, 0) and idx.tolist() == [2, 99, 3, -1]


def test_ops_on_cpu_tensors_take_the_reference_path(corpus):
    toks, offs = corpus.tokens.tensor().view(-1), corpus.offsets.tensor().view(-1)
    perm = FeistelPermutation(200, seed=7, epoch=2)
    used_seen = set()
    for S in (37, 100):
        for sel in (dict(perm=perm, base=40, count=48), dict(index=torch.tensor([5, 0, 199, 5, 17, 42])),
                    dict(base=190), dict(index=torch.zeros(0, dtype=torch.int64))):
            got = ops.ffd_index_device(offs, seq_len=S, **sel)
            n = got["index"].numel()
            idx, ffd_rows, in_order, used = ops.ref_ffd_index(offs, n, sel.get("index"), sel.get("perm"),
                                                              sel.get("base", 0), seq_len=S)
            assert list(got) == ["index", "counts"] and got["counts"].dtype == torch.int64
            assert torch.equal(got["index"], idx) and got["counts"].tolist() == [ffd_rows, in_order, used]
            used_seen.add(used)
            for labels in (False, True):
                a = ops.pack_tokens_indexed_device(toks, offs, seq_len=S, pad_id=9, pack_order="ffd", labels=labels,
                                                   **sel)
                b = ops.pack_tokens_indexed_device(toks, offs, seq_len=S, pad_id=9, labels=labels, index=idx,
                                                   max_rows=a["input_ids"].shape[0],
                                                   max_segs=a["cu_seqlens"].numel() - 1)
                assert list(a) == list(b)
                for k in a:
                    assert torch.equal(a[k], b[k]), k
                assert a["counts"].numel() == 4 and int(a["counts"][0]) == min(ffd_rows, in_order)
    assert used_seen == {0, 1}
    with pytest.raises(ValueError, match="4096"):
        ops.ffd_index_device(torch.arange(5000, dtype=torch.int64), seq_len=8)
    with pytest.raises(ValueError, match="pack_order"):
        ops.pack_tokens_indexed_device(toks, offs, seq_len=8, pack_order="best_fit")
    assert ops.device_plan_bytes(100, 300, 200, ffd=True) == ops.device_plan_bytes(100, 300, 200) + 800 + 32
    assert ops.device_plan_bytes(100, 300, 200, ffd=False) == ops.device_plan_bytes(100, 300, 200)


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("seq_len", [100, 256])
def test_ffd_device_batches_equal_the_host_ffd_plan(corpus, seq_len, world):
    rank = world - 1
    ref = list(_host_ffd(corpus, seq_len, rank, world, n_epochs=2))
    in_order = list(_loader(corpus, seq_len, rank, world, plan="device", n_epochs=2))
    dev = _ffd_device(corpus, seq_len, rank, world, n_epochs=2)
    assert dev.pack_order == "ffd_device" and dev.token_rows == "fixed" and dev.plan == "device"
    ms, bound = dev.layout.max_segments, min(seq_len, corpus.max_len)
    it = iter(dev)
    half = len(ref) // 4  # mid-epoch
    for g in range(half):
        same_as_host_plan(next(it), ref[g], "pack", ms, bound)
    sd = dev.state_dict()
    assert sd["kind"] == "indexed"
    # the checkpoint goes to the host-FFD loader, which hands its own back
    host = _host_ffd(corpus, seq_len, rank, world, n_epochs=2, resume_state=sd)
    hit = iter(host)
    for g in range(half, half + 2):
        b = next(hit)
        assert torch.equal(b["input_ids"], ref[g]["input_ids"]) and b["n_rows"] == ref[g]["n_rows"]
    back = _ffd_device(corpus, seq_len, rank, world, n_epochs=2, resume_state=host.state_dict())
    rest = list(back)
    assert len(rest) == len(ref) - half - 2
    fewer = 0
    for g, b in enumerate(rest, half + 2):
        same_as_host_plan(b, ref[g], "pack", ms, bound)
        assert int(b["n_rows"]) <= int(in_order[g]["n_rows"])  # never more rows than the in-order plan
        fewer += int(b["n_rows"]) < int(in_order[g]["n_rows"])
    assert fewer > 0
    st = back.stats()
    assert st["pack_order"] == "ffd_device" and st["plan"] == "device"
    assert "pack_order" not in _loader(corpus, seq_len, plan="device").stats()


def test_refused_settings(corpus):
    with pytest.raises(ValueError, match="plan='device', mode='pack'"):
        _loader(corpus, plan="host", pack_order="ffd_device")
    with pytest.raises(ValueError, match="plan='device', mode='pack'"):
        _loader(corpus, plan="device", mode="pad", pack_order="ffd_device")
    for kw in (dict(plan="host"), dict(plan="host", mode="pad"), dict(plan="device", mode="pad")):
        with pytest.raises(ValueError, match="max_rows"):
            _loader(corpus, max_rows=8, **kw)
    with pytest.raises(ValueError, match="max_rows"):
        _loader(corpus, plan="device", max_rows=0)
    big = SharedTokenSource.synthetic(f"ddl_amd_ffd_big_{np.random.randint(1 << 30)}", 8200, 0, 3, seed=3,
                                      token_dtype="uint16")
    try:
        for gb, world in ((4097, 1), (8194, 2)):
            with pytest.raises(ValueError, match="4096"):
                ddl_amd.ResidentTokenLoader(big, gb, 100, "pack", DDLEnv(rank=0, world_size=world), device="cpu",
                                            plan="device", pack_order="ffd_device")
        ddl_amd.ResidentTokenLoader(big, 8192, 100, "pack", DDLEnv(rank=1, world_size=2), device="cpu", plan="device",
                                    pack_order="ffd_device").close()
    finally:
        big.close()
    for dl in (ddl_amd.ZeroCopyTokenLoader,):  # the new value is ResidentTokenLoader's alone
        with pytest.raises(ValueError, match="pack_order"):
            dl(corpus, GB, 100, "pack", DDLEnv(), device="cpu", pack_order="ffd_device")


@pytest.mark.parametrize("pack_order", ["in_order", "ffd_device"])
def test_max_rows(corpus, pack_order):
    full = list(_loader(corpus, plan="device", pack_order=pack_order, n_epochs=1))
    need = [int(b["n_rows"]) for b in full]
    top = max(need)
    assert min(need) < top
    at = list(_loader(corpus, plan="device", pack_order=pack_order, n_epochs=1, max_rows=top))
    below = list(_loader(corpus, plan="device", pack_order=pack_order, n_epochs=1, max_rows=top - 1))
    ms = full[0]["cu_seqlens"].numel() - 1
    for a, b, f, r in zip(at, below, full, need):
        assert a["input_ids"].shape == (top, 100) and b["input_ids"].shape == (top - 1, 100)
        assert a["cu_seqlens"].numel() == b["cu_seqlens"].numel() == ms + 1
        assert int(a["n_rows"]) == r and torch.equal(a["cu_seqlens"], f["cu_seqlens"])
        for k in ("input_ids", "attention_mask", "position_ids", "segment_ids"):
            assert torch.equal(a[k], f[k][:top]), k  # the live rows, and padding behind them
        if r <= top - 1:
            assert int(b["n_rows"]) == r and torch.equal(b["input_ids"], f["input_ids"][:top - 1])
        else:  # the plan kernel's overflow contract
            assert int(b["n_rows"]) == -1 and int(b["n_tokens"]) == int(f["n_tokens"])
            assert not b["attention_mask"].any() and bool((b["segment_ids"] == -1).all())
            assert bool((b["input_ids"] == 0).all()) and not b["cu_seqlens"].any()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_ffd_order_arithmetic_under_asan_ubsan(tmp_path):
    """The kernel's steps (csrc/kernels/tokens_ffd.h), replayed on the host over exact-size heap buffers against a
    straight transcription of the definition: a plain executable, nothing preloaded."""
    run_host_check(tmp_path, "tokens_ffd_check", "tokens ffd check ok")
