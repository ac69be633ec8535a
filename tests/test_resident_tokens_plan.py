"""``ResidentTokenLoader(plan="device")`` on the CPU (the device-planned ops' reference path) against the host
plan, the device-planned ops on CPU tensors against the composed references, and the host check of the batch
descriptor kernel's index arithmetic."""

import shutil

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check

GB = 16
COUNT_KEYS = ("n_tokens", "n_rows", "n_seg")


@pytest.fixture(params=["int32", "uint16"])
def corpus(request):
    """Lengths 0..300: empty sequences, and sequences longer than either seq_len."""
    src = SharedTokenSource.synthetic(f"ddl_amd_rtp_{np.random.randint(1 << 30)}", 200, 0, 300, seed=3,
                                      vocab=65536, token_dtype=request.param)
    yield src
    src.close()


def _loader(corpus, seq_len=100, mode="pack", rank=0, world=1, **kw):
    kw.setdefault("seed", 4)
    return ddl_amd.ResidentTokenLoader(corpus, GB, seq_len, mode, DDLEnv(rank=rank, world_size=world), device="cpu",
                                       **kw)


def _host(corpus, *a, **kw):
    return _loader(corpus, *a, plan="host", token_rows="fixed", **kw)


def _device(corpus, *a, **kw):
    return _loader(corpus, *a, plan="device", **kw)


def same_as_host_plan(dev: dict, host: dict, mode: str, max_segments: int, bound: int) -> None:
    """A ``plan="device"`` batch against the ``plan="host", token_rows="fixed"`` batch of the same step."""
    want = set(host) | ({"n_seg"} if mode == "pack" else set())
    assert set(dev) == want
    for k in host:
        if k in COUNT_KEYS or k in ("cu_seqlens", "max_seqlen"):
            continue
        assert dev[k].dtype == host[k].dtype and dev[k].shape == host[k].shape, k
        assert torch.equal(dev[k].cpu(), host[k].cpu()), k
    for k in COUNT_KEYS:
        if k in dev:
            assert isinstance(dev[k], torch.Tensor) and dev[k].dim() == 0 and dev[k].dtype == torch.int64, k
    assert int(dev["n_tokens"]) == host["n_tokens"]
    if mode == "pad":
        return
    n_seg = host["cu_seqlens"].numel() - 1
    assert int(dev["n_rows"]) == host["n_rows"] and int(dev["n_seg"]) == n_seg
    cu = dev["cu_seqlens"].cpu()
    assert cu.dtype == torch.int32 and cu.numel() == max_segments + 1
    assert torch.equal(cu[:n_seg + 1], host["cu_seqlens"].cpu())
    assert bool((cu[n_seg + 1:] == host["n_tokens"]).all())
    assert type(dev["max_seqlen"]) is int and dev["max_seqlen"] == bound and bound >= host["max_seqlen"]


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
@pytest.mark.parametrize("mode", ["pad", "pack"])
@pytest.mark.parametrize("seq_len", [100, 256])
def test_device_plan_batches_equal_the_host_plan(corpus, seq_len, mode, rank, world):
    dev, host = _device(corpus, seq_len, mode, rank, world), _host(corpus, seq_len, mode, rank, world)
    assert dev.plan == "device" and host.plan == "host"
    assert dev.token_rows == ("fixed" if mode == "pack" else "exact")
    assert len(dev) == len(host) == 12
    for _ in range(2):  # two epochs: the round keys change
        got, ref = list(dev), list(host)
        assert len(got) == len(ref) == 12
        for a, b in zip(got, ref):
            same_as_host_plan(a, b, mode, dev.layout.max_segments, min(seq_len, corpus.max_len))
    st = dev.stats()
    assert st["plan"] == "device" and st["batches"] == 24 and st["handoff"] == "device"
    assert "plan" not in host.stats()  # the default mode's stats are what they were
    assert dev.timing()["host_us_per_step"] > 0
    dev.close()
    dev.close()  # a second close is harmless
    host.close()


def test_unshuffled_order_uses_the_identity_selector(corpus):
    dev, host = _device(corpus, 100, "pack", n_epochs=1), _host(corpus, 100, "pack", n_epochs=1)
    for dl in (dev, host):
        dl.order.shuffle = False
    got, ref = list(dev), list(host)
    assert len(got) == len(ref) == 12
    for a, b in zip(got, ref):
        same_as_host_plan(a, b, "pack", dev.layout.max_segments, 100)
    offs = corpus.offsets.tensor().view(-1)
    assert int(got[0]["n_tokens"]) == int(offs[GB])  # the first batch is sequences 0 .. GB - 1


def test_a_host_plan_checkpoint_resumes_under_the_device_plan_and_back(corpus):
    ms = _host(corpus, 100, "pack").layout.max_segments
    full = list(_host(corpus, 100, "pack", n_epochs=1))
    host = _host(corpus, 100, "pack", n_epochs=1)
    it = iter(host)
    for _ in range(3):
        next(it)
    sd = host.state_dict()
    assert sd["kind"] == "indexed" and sd["global_batch_cursor"] == 3
    dev = _device(corpus, 100, "pack", n_epochs=1, resume_state=sd)  # host-plan state -> device plan
    it = iter(dev)
    for g in (3, 4, 5):
        same_as_host_plan(next(it), full[g], "pack", ms, 100)
    back = dev.state_dict()
    assert back["kind"] == "indexed" and back["global_batch_cursor"] == 6
    rest = list(_host(corpus, 100, "pack", n_epochs=1, resume_state=back))  # and back
    assert len(rest) == 6
    for a, b in zip(rest, full[6:]):
        assert torch.equal(a["input_ids"], b["input_ids"]) and a["n_tokens"] == b["n_tokens"]
    # a device-plan checkpoint taken at W = 2 resumes at W = 4 under either plan
    two = _device(corpus, 100, "pack", 0, 2, n_epochs=1)
    it = iter(two)
    for _ in range(3):
        next(it)
    sd2 = two.state_dict()
    assert sd2["world_size"] == 2 and sd2["global_batch_cursor"] == 3
    ref = list(_host(corpus, 100, "pack", 1, 4, n_epochs=1))[3:]
    got = list(_device(corpus, 100, "pack", 1, 4, n_epochs=1, resume_state=sd2))
    assert len(got) == len(ref) == 9
    ms4 = _host(corpus, 100, "pack", 1, 4).layout.max_segments
    for a, b in zip(got, ref):
        same_as_host_plan(a, b, "pack", ms4, 100)
    live = _device(corpus, 100, "pack", 1, 4, n_epochs=1)
    live.load_state_dict(sd2)  # on a live loader
    same_as_host_plan(next(iter(live)), ref[0], "pack", ms4, 100)


def test_refused_settings(corpus):
    with pytest.raises(ValueError, match="host plan"):
        _device(corpus, 100, "pack", pack_order="ffd")
    with pytest.raises(ValueError, match="fixed"):
        _device(corpus, 100, "pack", token_rows="exact")
    with pytest.raises(ValueError, match="plan must be"):
        _loader(corpus, 100, "pack", plan="gpu")
    _device(corpus, 100, "pad", token_rows="exact").close()  # pad mode has one row per sequence either way
    _device(corpus, 100, "pack", token_rows="fixed").close()

    class Huge:  # a corpus whose batches could overflow int32 cu_seqlens: refused at construction
        def __getattr__(self, name):
            return getattr(corpus, name)

        max_len = (0x7FFFFFFF // GB) + 1

    with pytest.raises(ValueError, match="int32 cu_seqlens"):
        ddl_amd.ResidentTokenLoader(Huge(), GB, 100, "pack", DDLEnv(), device="cpu", plan="device")


@pytest.mark.parametrize("position_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("seq_len", [6, 100])
def test_device_planned_ops_on_cpu_tensors_equal_the_composed_references(corpus, seq_len, position_dtype):
    toks = corpus.tokens.tensor().view(-1)
    offs = corpus.offsets.tensor().view(-1)
    perm = FeistelPermutation(200, seed=7, epoch=2)
    selections = [(dict(index=torch.tensor([5, 0, 199, 5, 17, 42])), [5, 0, 199, 5, 17, 42]),
                  (dict(index=torch.zeros(0, dtype=torch.int64)), []),
                  (dict(perm=perm, base=40, count=33), perm(np.arange(40, 73)).tolist()),
                  (dict(base=190), list(range(190, 200))),
                  (dict(base=3, count=4), [3, 4, 5, 6])]
    for sel, idx in selections:
        idx = np.asarray(idx, dtype=np.int64)
        flat, dofs = ops.ref_gather_ragged(toks, offs, idx)
        n_tokens = int(dofs[-1])
        lens = np.diff(dofs.numpy())
        max_seg = int(min(lens.max(), seq_len)) if len(idx) else 0
        got = ops.pad_tokens_indexed_device(toks, offs, seq_len=seq_len, pad_id=9, position_dtype=position_dtype,
                                            **sel)
        ref = ops.ref_pad_tokens(flat, dofs, seq_len, 9, position_dtype)
        assert list(got) == ["input_ids", "attention_mask", "position_ids", "counts"]
        for k, b in zip(got, ref):
            assert got[k].dtype == b.dtype and torch.equal(got[k], b), k
        assert got["counts"].tolist() == [len(idx), 0, n_tokens, max_seg]

        rs, re_, so = ops.ref_pack_plan(dofs.numpy(), seq_len)
        n_seg = len(so) - 1
        for caps in ({}, dict(max_rows=len(rs) + 2, max_segs=n_seg + 5), dict(max_rows=max(len(rs), 1),
                                                                              max_segs=max(n_seg, 1))):
            got = ops.pack_tokens_indexed_device(toks, offs, seq_len=seq_len, pad_id=9, position_dtype=position_dtype,
                                                 **sel, **caps)
            R, M = got["input_ids"].shape[0], got["cu_seqlens"].numel() - 1
            if caps:
                assert (R, M) == (caps["max_rows"], caps["max_segs"])
            assert R >= len(rs) and M >= n_seg
            ref = ops.ref_pack_tokens(flat, rs, re_, so, seq_len, 9, position_dtype, fill_rows=R)
            assert list(got) == ["input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "counts"]
            for k, b in zip(got, ref):
                assert got[k].dtype == b.dtype and got[k].shape == (R, seq_len) and torch.equal(got[k], b), k
            cu = got["cu_seqlens"]
            assert cu.dtype == torch.int32 and cu[:n_seg + 1].tolist() == so.tolist()
            assert bool((cu[n_seg + 1:] == n_tokens).all())
            assert got["counts"].dtype == torch.int64
            assert got["counts"].tolist() == [len(rs), n_seg, n_tokens, max_seg]
    # a capacity that is too small: n_rows = -1, every row padding, cu_seqlens zero
    got = ops.pack_tokens_indexed_device(toks, offs, perm=perm, base=0, count=64, seq_len=seq_len, pad_id=9,
                                         max_rows=2, max_segs=4000)
    assert got["counts"][0].item() == -1 and got["counts"][2].item() > 0
    assert bool((got["input_ids"] == 9).all()) and bool((got["segment_ids"] == -1).all())
    assert not got["attention_mask"].any() and not got["cu_seqlens"].any()
    with pytest.raises(IndexError):
        ops.pack_tokens_indexed_device(toks, offs, base=195, count=6, seq_len=seq_len)
    with pytest.raises(IndexError):
        ops.pad_tokens_indexed_device(toks, offs, perm=perm, base=190, count=11, seq_len=seq_len)
    with pytest.raises(ValueError):
        ops.pad_tokens_indexed_device(toks, offs, index=torch.tensor([1]), perm=perm, seq_len=seq_len)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_batch_descriptor_arithmetic_under_asan_ubsan(tmp_path):
    """The kernel's per-lane loops (csrc/kernels/tokens_plan.h), replayed on the host over exact-size heap buffers
    for the corpus offsets, the index and the outputs, indices outside the corpus and capacities that are too
    small included: a plain executable, nothing preloaded."""
    run_host_check(tmp_path, "tokens_plan_check", "tokens plan check ok")
