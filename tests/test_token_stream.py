"""The token stream format on the CPU: ``ops.ref_stream_tokens`` (the definition) against a per-token loop, the
capacity of ``ops.stream_max_segments``, the overflow convention, ``ResidentTokenStreamLoader``'s CPU twin (world
sizes, epochs, checkpoints) and the host replay of the stream kernels' index arithmetic."""

import shutil

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.ops.kernels import widen_tokens
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check

KEYS = ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens")


def _corpus(lens, seed=0, vocab=50000):
    lens = np.asarray(lens, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = np.random.default_rng(seed).integers(1, vocab, size=int(offs[-1]), dtype=np.int32)
    return torch.from_numpy(toks), torch.from_numpy(offs)


def brute_force(toks, offs, order, row_base, rows, S, pad_id, max_segs, ignore_index):
    """The definition, one token at a time."""
    stream = []  # (token, document)
    for d in order:
        stream += [(int(toks[p]), d) for p in range(int(offs[d]), int(offs[d + 1]))]
    ids = [[pad_id] * S for _ in range(rows)]
    mask = [[0] * S for _ in range(rows)]
    pos = [[0] * S for _ in range(rows)]
    seg = [[-1] * S for _ in range(rows)]
    lab = [[ignore_index] * S for _ in range(rows)]
    cu, n_seg, n_tok, max_seg, n_rows = [], 0, 0, 0, 0
    for r in range(rows):
        prev, run = None, 0
        for p in range(S):
            g = (row_base + r) * S + p
            if g >= len(stream):
                break
            tok, d = stream[g]
            if d != prev:
                cu.append(n_tok)
                n_seg, prev, run = n_seg + 1, d, 0
            ids[r][p], mask[r][p], pos[r][p], seg[r][p] = tok, 1, run, n_seg - 1
            if p and seg[r][p - 1] == n_seg - 1:
                lab[r][p - 1] = tok
            run, n_tok, n_rows = run + 1, n_tok + 1, r + 1
            max_seg = max(max_seg, run)
    cu = cu + [n_tok] * (max_segs + 1 - len(cu))
    return dict(input_ids=ids, attention_mask=mask, position_ids=pos, segment_ids=seg, cu_seqlens=cu, labels=lab,
                counts=[n_rows, n_seg, n_tok, max_seg])


@pytest.mark.parametrize("S", [4, 6])
def test_reference_equals_a_per_token_loop(S):
    lens = [0, 1, S, S + 1, 3 * S + 2, 2, 0]
    toks, offs = _corpus(lens, seed=S)
    T = sum(lens)
    perm = FeistelPermutation(7, seed=3, epoch=1)
    for p in (None, perm):
        order = list(range(7)) if p is None else p(np.arange(7)).tolist()
        for rows in (1, 2, 3):
            for row_base in range(0, T // S + 3):
                for pdt in (torch.int64, torch.int32):
                    got = ops.ref_stream_tokens(toks, offs, perm=p, row_base=row_base, rows=rows, seq_len=S,
                                                pad_id=7, position_dtype=pdt, max_segs=12, labels=True,
                                                ignore_index=-5)
                    want = brute_force(toks, offs, order, row_base, rows, S, 7, 12, -5)
                    assert list(got) == [*KEYS, "counts", "labels"]
                    for k in want:
                        assert got[k].tolist() == want[k], (k, rows, row_base)
                    assert got["input_ids"].dtype == torch.int32 and got["attention_mask"].dtype == torch.uint8
                    assert got["position_ids"].dtype == pdt and got["segment_ids"].dtype == torch.int32
                    assert got["cu_seqlens"].dtype == torch.int32 and got["counts"].dtype == torch.int64
                    assert got["labels"].dtype == torch.int64
    # the op on CPU tensors is the reference, and a 16-bit corpus widens
    a = ops.stream_tokens_indexed_device(toks, offs, perm=perm, row_base=1, rows=2, seq_len=S, max_segs=9)
    b = ops.ref_stream_tokens(toks.to(torch.int16), offs, perm=perm, row_base=1, rows=2, seq_len=S, max_segs=9)
    for k in (*KEYS, "counts"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ops.token_stream_table(offs, perm),
                       torch.from_numpy(np.concatenate([[0], np.cumsum(np.asarray(lens)[perm(np.arange(7))])])))


def test_no_window_of_any_order_exceeds_stream_max_segments():
    rng = np.random.default_rng(11)
    for case in range(200):
        S = int(rng.integers(1, 40))
        n = int(rng.integers(1, 301))
        lens = rng.integers(0, 3 * S + 1, size=n)
        if case % 5 == 0:
            lens[rng.random(n) < 0.5] = 0
        if case % 7 == 0:
            lens = np.minimum(lens, 2)  # many short documents: the count of documents is what binds
        toks, offs = _corpus(lens, seed=case, vocab=100)
        T = int(lens.sum())
        rows = int(rng.integers(1, 9))
        perm = FeistelPermutation(n, seed=case, epoch=case % 3) if case % 2 else None
        cap = ops.stream_max_segments(lens, rows, S)
        for row_base in {0, int(rng.integers(0, T // S + 2)), int(rng.integers(0, T // S + 2)), max(T // S - rows, 0)}:
            r = ops.ref_stream_tokens(toks, offs, perm=perm, row_base=row_base, rows=rows, seq_len=S)
            n_seg = int(r["counts"][1])
            assert n_seg <= cap, (case, S, n, rows, row_base, n_seg, cap)
            assert int(r["counts"][0]) >= 0  # the default capacity of the op never overflows either
            # and a batch is rendered the same at the tight capacity
            t = ops.ref_stream_tokens(toks, offs, perm=perm, row_base=row_base, rows=rows, seq_len=S, max_segs=cap)
            assert torch.equal(t["input_ids"], r["input_ids"]) and torch.equal(t["counts"], r["counts"])


def test_overflow_convention():
    S = 6
    toks, offs = _corpus([0, 1, S, S + 1, 3 * S + 2, 2, 0])
    full = ops.ref_stream_tokens(toks, offs, row_base=0, rows=3, seq_len=S, pad_id=9, labels=True)
    n_rows, n_seg, n_tok, max_seg = full["counts"].tolist()
    assert n_rows == 3 and n_seg == 6 and n_tok == 18
    fit = ops.ref_stream_tokens(toks, offs, row_base=0, rows=3, seq_len=S, pad_id=9, max_segs=n_seg, labels=True)
    assert torch.equal(fit["input_ids"], full["input_ids"]) and fit["cu_seqlens"].numel() == n_seg + 1
    over = ops.ref_stream_tokens(toks, offs, row_base=0, rows=3, seq_len=S, pad_id=9, max_segs=n_seg - 1,
                                 labels=True, ignore_index=-7)
    assert over["counts"].tolist() == [-1, n_seg, n_tok, max_seg]
    assert bool((over["input_ids"] == 9).all()) and bool((over["segment_ids"] == -1).all())
    assert not over["attention_mask"].any() and not over["position_ids"].any()
    assert over["cu_seqlens"].numel() == n_seg and not over["cu_seqlens"].any()
    assert bool((over["labels"] == -7).all())
    with pytest.raises(ValueError, match="int32 cu_seqlens"):
        ops.stream_tokens_indexed_device(toks, offs, row_base=0, rows=1 << 20, seq_len=1 << 12)


@pytest.fixture(scope="module")
def source():
    src = SharedTokenSource.synthetic(f"ddl_amd_ts_{np.random.randint(1 << 30)}", 300, 0, 90, seed=5, vocab=65536,
                                      token_dtype="uint16")
    yield src
    src.close()


GB, S = 8, 32


def _loader(source, rank=0, world=1, **kw):
    kw.setdefault("seed", 4)
    return ddl_amd.ResidentTokenStreamLoader(source, GB, S, DDLEnv(rank=rank, world_size=world), device="cpu", **kw)


def _same_batch(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_cpu_twin_batches_follow_the_definition(source):
    dl = _loader(source, labels=True)
    toks, offs = source.tokens.tensor().view(-1), source.offsets.tensor().view(-1)
    T = int(offs[-1])
    assert dl.total_tokens == T and dl.order.n_samples == T // S and len(dl) == T // S // GB
    assert dl.max_segments == ops.stream_max_segments(np.diff(offs.numpy()), GB, S)
    batches = list(dl)
    assert len(batches) == T // S // GB
    for g, b in enumerate(batches):
        assert list(b) == [*KEYS, "labels", "max_seqlen", "n_tokens", "n_rows", "n_seg"]
        ref = ops.ref_stream_tokens(toks, offs, perm=FeistelPermutation(300, 4, 0), row_base=g * GB, rows=GB,
                                    seq_len=S, max_segs=dl.max_segments, labels=True)
        for k in (*KEYS, "labels"):
            assert torch.equal(b[k], ref[k]), k
        assert b["input_ids"].shape == (GB, S) and bool(b["attention_mask"].all())  # 100% dense
        assert b["max_seqlen"] == min(S, source.max_len) and type(b["max_seqlen"]) is int
        for k, i in (("n_rows", 0), ("n_seg", 1), ("n_tokens", 2)):
            assert b[k].dim() == 0 and b[k].dtype == torch.int64 and int(b[k]) == int(ref["counts"][i])
        assert int(b["n_tokens"]) == GB * S and int(b["n_rows"]) == GB
    # the epoch's rows are the stream itself, in order
    order = FeistelPermutation(300, 4, 0)(np.arange(300))
    stream = torch.cat([widen_tokens(toks[int(offs[q]):int(offs[q + 1])]) for q in order])
    got = torch.cat([b["input_ids"].reshape(-1) for b in batches])
    assert torch.equal(got, stream[:got.numel()]) and stream.numel() - got.numel() < GB * S
    st = dl.stats()
    assert st["format"] == "stream" and st["batches"] == len(batches) and dl.timing()["host_us_per_step"] > 0
    dl.close()
    dl.close()


def test_union_of_ranks_is_the_same_at_every_world_size(source):
    ref = [b["input_ids"] for b in _loader(source, n_epochs=1)]
    for world in (2, 4, 8):
        per_rank = [[b["input_ids"] for b in _loader(source, r, world, n_epochs=1)] for r in range(world)]
        assert all(len(p) == len(ref) for p in per_rank)
        for g, want in enumerate(ref):
            assert torch.equal(torch.cat([p[g] for p in per_rank]), want), (world, g)
    with pytest.raises(ValueError, match="divisible"):
        _loader(source, 0, 3)


def test_epochs_differ_when_shuffled_and_are_equal_when_not(source):
    dl = _loader(source)
    e0, e1 = list(dl), list(dl)
    assert len(e0) == len(e1) and dl.epoch == 2
    assert any(not torch.equal(a["input_ids"], b["input_ids"]) for a, b in zip(e0, e1))
    plain = _loader(source, shuffle=False)
    p0, p1 = list(plain), list(plain)
    for a, b in zip(p0, p1):
        _same_batch(a, b)
    toks, offs = source.tokens.tensor().view(-1), source.offsets.tensor().view(-1)
    first = widen_tokens(toks[:GB * S]).view(GB, S)  # unshuffled: the corpus itself, cut every S tokens
    assert torch.equal(p0[0]["input_ids"], first)
    with pytest.raises(ValueError, match="fewer than one global batch"):
        ddl_amd.ResidentTokenStreamLoader(source, 1 << 20, S, DDLEnv(), device="cpu")


def test_checkpoint_resumes_at_another_world_size_and_refuses_other_kinds(source):
    full = [b["input_ids"] for b in _loader(source, n_epochs=1)]
    two = _loader(source, 0, 2, n_epochs=1)
    it = iter(two)
    for _ in range(3):
        next(it)
    sd = two.state_dict()
    assert sd["kind"] == "token_stream" and sd["world_size"] == 2 and sd["global_batch_cursor"] == 3
    for k, v in (("seq_len", S), ("n_documents", 300), ("total_tokens", two.total_tokens), ("global_batch", GB),
                 ("order_seed", 4), ("epoch", 0)):
        assert sd[k] == v, k
    ranks = [list(_loader(source, r, 4, n_epochs=1, resume_state=sd)) for r in range(4)]
    assert all(len(r) == len(full) - 3 for r in ranks)
    for g in range(3, len(full)):
        assert torch.equal(torch.cat([r[g - 3]["input_ids"] for r in ranks]), full[g]), g
    live = _loader(source, 1, 4, n_epochs=1)
    live.load_state_dict(sd)  # on a live loader
    assert torch.equal(next(iter(live))["input_ids"], full[3][2:4])
    # the two kinds of cursor do not mix, in either direction
    indexed = ddl_amd.ResidentTokenLoader(source, GB, S, "pack", DDLEnv(), device="cpu", seed=4)
    with pytest.raises(ValueError, match="token stream"):
        _loader(source, resume_state=indexed.state_dict())
    with pytest.raises(ValueError, match="token stream"):
        live.load_state_dict(indexed.state_dict())
    with pytest.raises(ValueError, match="indexed"):
        indexed.load_state_dict(sd)
    with pytest.raises(ValueError, match="seq_len"):
        ddl_amd.ResidentTokenStreamLoader(source, GB, S * 2, DDLEnv(), device="cpu", seed=4, resume_state=sd)
    indexed.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_stream_kernel_arithmetic_under_asan_ubsan(tmp_path):
    """The kernels' per-lane loops (csrc/kernels/tokens_stream.h), replayed on the host over exact-size heap
    buffers for the corpus offsets, the order, the table and the plan arrays, indices outside the corpus and
    capacities that are too small included: a plain executable, nothing preloaded."""
    run_host_check(tmp_path, "tokens_stream_check", "tokens stream check ok")
