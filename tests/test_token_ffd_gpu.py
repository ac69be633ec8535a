"""``token_ffd_order`` on the GPU against its definition (``ops.ref_ffd_index``), bit for bit, over the smallest
shapes at which it can go wrong, and the paths built on it: ``pack_tokens_indexed_device(pack_order="ffd")``
against its CPU path, ``ResidentTokenLoader(pack_order="ffd_device")`` against the host FFD plan, ``max_rows``,
and a corpus whose offsets pass 2^32. The kernel reads lengths only (no token), so the token width enters with the
end-to-end tests."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.types import DDLEnv
from tests.test_resident_tokens_plan import same_as_host_plan

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4096)
N_CORPUS = 5000
BASE = 700  # of the permutation and identity selectors


def _patterns(n: int, S: int, rng) -> dict:
    """The batch's lengths, by name."""
    i = np.arange(n)
    special = np.array([0, S, 2 * S, S + 1, 3 * S - 1])
    out = {"all equal": np.full(n, S // 3 + 1),
           "special mixed in": np.where(i % 3 == 0, special[(i // 3) % 5], rng.integers(1, S + 1, n)),
           "long with tiny remainders": np.where(i % 4 == 0, S * (1 + i % 3) + 1 + i % 2,
                                                 rng.integers(1, S // 2 + 1, n)),
           "in-order pairs": np.where(i % 2 == 0, S - S // 2, S // 2),
           "random in [1, 2S]": rng.integers(1, 2 * S + 1, n)}
    if n == 1025:  # once per S: the second level of the tree, and all of it
        out["200 bins"] = np.full(200, S // 2 + 1)
        out["the full tree"] = np.full(4096, S // 2 + 1)
    return out


def _case(lens: np.ndarray, selector: str, rng):
    """(corpus offsets, the selector's arguments) of a batch with these lengths."""
    n = len(lens)
    corpus = rng.integers(0, 50, N_CORPUS)
    if selector == "index":
        q = rng.permutation(N_CORPUS)[:n].astype(np.int64)
        corpus[q] = lens
        if n > 1:
            q[n // 2] = N_CORPUS + 3 if n % 2 else -1  # outside the corpus: an empty sequence
        sel = dict(index=torch.from_numpy(q))
    elif selector == "perm":
        perm = FeistelPermutation(N_CORPUS, seed=11, epoch=3)
        corpus[perm(np.arange(BASE, BASE + n))] = lens
        sel = dict(perm=perm, base=BASE, count=n)
    else:
        corpus[BASE:BASE + n] = lens
        sel = dict(base=BASE, count=n)
    offs = np.concatenate([[0], np.cumsum(corpus)]).astype(np.int64)
    return torch.from_numpy(offs), sel


def _on_gpu(sel: dict) -> dict:
    return {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in sel.items()}


@pytest.mark.parametrize("selector", ["perm", "index", "identity"])
@pytest.mark.parametrize("S", [8, 37, 4096])
def test_index_and_counts_equal_the_definition_bit_for_bit(S, selector):
    rng = np.random.default_rng(S)
    used_seen = {0: 0, 1: 0}
    for n in SIZES:
        for name, lens in _patterns(n, S, rng).items():
            offs, sel = _case(lens, selector, rng)
            m = len(lens)
            idx, ffd_rows, in_order, used = ops.ref_ffd_index(offs, m, sel.get("index"), sel.get("perm"),
                                                              sel.get("base", 0), seq_len=S)
            used_seen[used] += 1
            got = ops.ffd_index_device(offs.cuda(), seq_len=S, **_on_gpu(sel))
            assert got["index"].dtype == got["counts"].dtype == torch.int64
            assert got["counts"].tolist() == [ffd_rows, in_order, used], (name, n)
            assert torch.equal(got["index"].cpu(), idx), (name, n)
    assert used_seen[0] > 0 and used_seen[1] > 0  # a kernel that always falls back cannot pass


def test_out_buffer_and_refusals():
    offs = torch.arange(0, 6 * 5001, 6, dtype=torch.int64).cuda()
    out = torch.full((40,), -7, dtype=torch.int64, device="cuda")
    got = ops.ffd_index_device(offs, base=3, count=20, seq_len=8, out=out)
    assert got["index"].data_ptr() == out.data_ptr() and got["counts"].data_ptr() == out.data_ptr() + 160
    assert sorted(got["index"].tolist()) == list(range(3, 23)) and bool((out[23:] == -7).all())
    with pytest.raises(ValueError, match="4096"):
        ops.ffd_index_device(offs, count=4097, seq_len=8)
    with pytest.raises(ValueError):
        ops.ffd_index_device(offs, count=20, seq_len=8, out=out[:22])


def test_offsets_past_2_to_32():
    """Documents of 2^33 tokens and more among short ones: only the offsets exist (the kernel reads no token)."""
    big = 1 << 33
    lens = np.array([5, big + 3, 0, 7, 3 * big, big, 1, (1 << 32) + 3, 4097, 2 * big + 4095, 11, big - 1] * 6)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    assert int(offs[-1]) > 1 << 38
    q = torch.from_numpy(np.random.default_rng(5).permutation(len(lens)).astype(np.int64))
    seen = set()
    for S in (1 << 22, 1 << 31, (1 << 33) + 1):  # rows long enough that the reference's chunk loop stays short
        idx, ffd_rows, in_order, used = ops.ref_ffd_index(offs, len(q), q, seq_len=S)
        got = ops.ffd_index_device(offs.cuda(), index=q.cuda(), seq_len=S)
        assert got["counts"].tolist() == [ffd_rows, in_order, used] and torch.equal(got["index"].cpu(), idx)
        seen.add(used)
    assert 1 in seen


@pytest.fixture(params=["int32", "uint16"])
def corpus(request):
    src = SharedTokenSource.synthetic(f"ddl_amd_ffdg_{np.random.randint(1 << 30)}", 1100, 0, 300, seed=3,
                                      vocab=65536, token_dtype=request.param)
    yield src
    src.close()


@pytest.mark.parametrize("labels", [False, True])
def test_pack_op_with_ffd_equals_its_cpu_path(corpus, labels):
    toks, offs = corpus.tokens.tensor().view(-1), corpus.offsets.tensor().view(-1)
    perm = FeistelPermutation(1100, seed=7, epoch=2)
    q = torch.from_numpy(np.random.default_rng(1).integers(0, 1100, 70))
    for S in (37, 100):
        for sel in (dict(perm=perm, base=40, count=333), dict(index=q), dict(base=1000),
                    dict(index=torch.zeros(0, dtype=torch.int64))):
            kw = dict(seq_len=S, pad_id=9, pack_order="ffd", labels=labels)
            ref = ops.pack_tokens_indexed_device(toks, offs, **sel, **kw)
            got = ops.pack_tokens_indexed_device(toks.cuda(), offs.cuda(), **_on_gpu(sel), **kw)
            assert list(got) == list(ref)
            for k in ref:
                assert got[k].dtype == ref[k].dtype and torch.equal(got[k].cpu(), ref[k]), (k, S)
            plain = ops.pack_tokens_indexed_device(toks, offs, **sel, seq_len=S, pad_id=9)
            assert int(ref["counts"][0]) <= int(plain["counts"][0])


def _pair(corpus, gb, seq_len, **kw):
    env = DDLEnv(rank=0, world_size=1)
    dev = ddl_amd.ResidentTokenLoader(corpus, gb, seq_len, "pack", env, seed=4, n_epochs=2, plan="device",
                                      pack_order="ffd_device", **kw)
    host = ddl_amd.ResidentTokenLoader(corpus, gb, seq_len, "pack", env, seed=4, n_epochs=2, plan="host",
                                       pack_order="ffd", token_rows="fixed", device="cpu",
                                       labels=kw.get("labels", False))
    return dev, host


@pytest.mark.parametrize("gb", [100, 256])
def test_loader_equals_the_host_ffd_loader(corpus, gb):
    dev, host = _pair(corpus, gb, 100, labels=gb == 100)
    try:
        per_epoch = 1100 // gb
        got, ref = list(dev), list(host)  # one epoch
        assert len(got) == len(ref) == per_epoch
        it, rit = iter(dev), iter(host)  # and the first batches behind the boundary
        got += [next(it), next(it)]
        ref += [next(rit), next(rit)]
        for a, b in zip(got, ref):
            same_as_host_plan(a, b, "pack", dev.layout.max_segments, 100)
        assert dev.stats()["pack_order"] == "ffd_device"
    finally:
        dev.close()
        host.close()


def test_max_rows_on_the_gpu(corpus):
    env = DDLEnv(rank=0, world_size=1)
    kw = dict(seed=4, n_epochs=1, plan="device", pack_order="ffd_device")
    twin = list(ddl_amd.ResidentTokenLoader(corpus, 100, 100, "pack", env, device="cpu", **kw))
    need = [int(b["n_rows"]) for b in twin]
    top = max(need)
    assert min(need) < top
    for rows in (top, top - 1):
        dl = ddl_amd.ResidentTokenLoader(corpus, 100, 100, "pack", env, max_rows=rows, **kw)
        ref = list(ddl_amd.ResidentTokenLoader(corpus, 100, 100, "pack", env, device="cpu", max_rows=rows, **kw))
        try:
            got = list(dl)
            assert len(got) == len(ref) == len(need)
            for a, b, r in zip(got, ref, need):
                assert a["input_ids"].shape == (rows, 100)
                assert int(a["n_rows"]) == (r if r <= rows else -1) == int(b["n_rows"])
                for k in ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens"):
                    assert torch.equal(a[k].cpu(), b[k]), k
        finally:
            dl.close()
