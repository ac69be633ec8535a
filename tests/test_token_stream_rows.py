"""Shuffled rows of the token stream on the CPU: ``ops.ref_stream_tokens(row_perm= / row_index=)`` against a
construction that materialises the stream and slices its rows, the segment bound against a brute-force count,
the invalid-row and overflow conventions, the loader's CPU twin (every row of an epoch once, the same batches at
every world size, checkpoints) and the host replay of the row plan kernels under ASan/UBSan."""

import shutil

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.ops.kernels import widen_tokens
from ddl_amd.permutation import FeistelPermutation, row_seed_for
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check

KEYS = ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "counts")


def _corpus(lens, seed=0, vocab=50000):
    lens = np.asarray(lens, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = np.random.default_rng(seed).integers(1, vocab, size=int(offs[-1]), dtype=np.int32)
    return torch.from_numpy(toks), torch.from_numpy(offs)


def _stream(toks, offs, order):
    """The stream and, per token, the document it comes from."""
    o = offs.numpy()
    stream = np.concatenate([toks.numpy()[o[q]:o[q + 1]] for q in order] + [np.zeros(0, dtype=np.int32)])
    doc = np.concatenate([np.full(o[q + 1] - o[q], i) for i, q in enumerate(order)] + [np.zeros(0, dtype=np.int64)])
    return stream, doc


def _by_slicing(toks, offs, order, rho, S, max_segs):
    """Materialise the stream, slice the rows; segments by a per-token loop. Valid rows only."""
    stream, doc = _stream(toks, offs, order)
    ids = np.stack([stream[r * S:(r + 1) * S] for r in rho])
    docs = np.stack([doc[r * S:(r + 1) * S] for r in rho])
    pos, sid, cu = np.zeros_like(ids, dtype=np.int64), np.zeros_like(ids), []
    for k in range(len(rho)):
        for p in range(S):
            if p == 0 or docs[k, p] != docs[k, p - 1]:
                cu.append(k * S + p)
            pos[k, p] = k * S + p - cu[-1]
            sid[k, p] = len(cu) - 1
    n_seg = len(cu)
    mx = int(np.diff(cu + [len(rho) * S]).max())
    cu = np.array(cu + [len(rho) * S] * (max_segs + 1 - n_seg), dtype=np.int32)
    return ids, pos, sid, cu, [len(rho), n_seg, len(rho) * S, mx]


@pytest.mark.parametrize("S", [4, 7, 32])
def test_definition_equals_slicing_the_materialised_stream(S):
    rng = np.random.default_rng(S)
    lens = rng.choice([0, 0, 1, 2, S - 1, S, S + 1, 3 * S + 2], size=60)
    toks, offs = _corpus(lens, seed=S)
    n, T = 60, int(offs[-1])
    n_rows = T // S
    for perm in (None, FeistelPermutation(n, 3, 1)):
        order = np.arange(n) if perm is None else perm(np.arange(n))
        row_perm = FeistelPermutation(n_rows, 11, 2)
        selections = [
            dict(row_perm=row_perm, row_base=0), dict(row_perm=row_perm, row_base=n_rows - 5),
            dict(row_index=torch.from_numpy(rng.permutation(n_rows)[:5].astype(np.int64)), row_base=0),
            dict(row_index=np.array([2, 0, 2, 2, n_rows - 1], dtype=np.int64), row_base=0),  # a row three times
        ]
        for sel in selections:
            rho = (row_perm(np.arange(sel["row_base"], sel["row_base"] + 5)) if "row_perm" in sel
                   else np.asarray(sel["row_index"]))
            M = 5 * S
            got = ops.ref_stream_tokens(toks, offs, perm=perm, rows=5, seq_len=S, max_segs=M, labels=True, **sel)
            ids, pos, sid, cu, counts = _by_slicing(toks, offs, order, rho, S, M)
            assert np.array_equal(got["input_ids"].numpy(), ids)
            assert bool(got["attention_mask"].all())
            assert np.array_equal(got["position_ids"].numpy(), pos)
            assert np.array_equal(got["segment_ids"].numpy(), sid)
            assert np.array_equal(got["cu_seqlens"].numpy(), cu)
            assert got["counts"].tolist() == counts
            assert torch.equal(got["labels"], ops.ref_token_labels(got["input_ids"], got["attention_mask"],
                                                                   got["segment_ids"], -100))


def test_an_arange_row_index_equals_the_contiguous_rows():
    lens = np.random.default_rng(1).choice([0, 1, 5, 6, 7, 20], size=80)
    toks, offs = _corpus(lens)
    S, rows = 6, 4
    perm = FeistelPermutation(80, 2, 0)
    for b in (0, 3, int(offs[-1]) // S - rows):
        kw = dict(perm=perm, rows=rows, seq_len=S, max_segs=40, labels=True, position_dtype=torch.int32)
        want = ops.ref_stream_tokens(toks, offs, row_base=b, **kw)
        got = ops.ref_stream_tokens(toks, offs, row_base=0, row_index=np.arange(b, b + rows, dtype=np.int64), **kw)
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_refused_selections():
    toks, offs = _corpus([5, 9, 3, 12])
    kw = dict(rows=2, seq_len=4)
    with pytest.raises(ValueError, match="not both"):
        ops.ref_stream_tokens(toks, offs, row_base=0, row_perm=FeistelPermutation(7, 0, 0),
                              row_index=np.zeros(2, dtype=np.int64), **kw)
    with pytest.raises(ValueError, match="row_base"):
        ops.ref_stream_tokens(toks, offs, row_base=1, row_index=np.zeros(2, dtype=np.int64), **kw)
    with pytest.raises(ValueError, match="entries"):
        ops.ref_stream_tokens(toks, offs, row_base=0, row_index=np.zeros(3, dtype=np.int64), **kw)
    with pytest.raises(TypeError):
        ops.ref_stream_tokens(toks, offs, row_base=0, row_index=np.zeros(2, dtype=np.int32), **kw)
    with pytest.raises(IndexError):
        ops.ref_stream_tokens(toks, offs, row_base=6, row_perm=FeistelPermutation(7, 0, 0), **kw)
    with pytest.raises(IndexError, match="full rows"):  # the op checks the domain: T // S = 7
        ops.stream_tokens_indexed_device(toks, offs, row_base=0, row_perm=FeistelPermutation(6, 0, 0), **kw)
    got = ops.stream_tokens_indexed_device(toks, offs, row_base=0, row_perm=FeistelPermutation(7, 0, 0), **kw)
    want = ops.ref_stream_tokens(toks, offs, row_base=0, row_perm=FeistelPermutation(7, 0, 0), **kw)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert got["cu_seqlens"].numel() == min(min(4, 8) + 4, 8) + 1  # the length-free default capacity


def _brute_segments(lens, rho, S):
    """Segments of the rows ``rho`` of the stream of documents ``lens``: a per-token count."""
    doc = np.repeat(np.arange(len(lens)), lens)
    return sum(1 + int(np.count_nonzero(np.diff(doc[r * S:(r + 1) * S]))) for r in rho)


def test_no_distinct_rows_exceed_the_shuffled_bound_and_some_reach_it():
    rng = np.random.default_rng(7)
    reached = 0
    for case in range(4000):
        S = int(rng.integers(2, 9))
        n = int(rng.integers(1, 31))
        lens = rng.integers(0, 3 * S, size=n) * (rng.random(n) < 0.8)
        T = int(lens.sum())
        if T // S < 1:
            continue
        rows = int(rng.integers(1, min(4, T // S) + 1))
        rho = rng.permutation(T // S)[:rows]
        bound = ops.stream_max_segments(lens, rows, S, shuffled_rows=True)
        nonempty = np.sort(lens[lens > 0])
        k = int(np.searchsorted(np.cumsum(nonempty), rows * S, side="right"))
        assert bound == max(1, min(k, nonempty.size) + 2 * rows)
        count = _brute_segments(lens, rho, S)
        assert count <= bound, (lens.tolist(), rho.tolist(), S)
        toks, offs = _corpus(lens)
        ref = ops.ref_stream_tokens(toks, offs, row_base=0, rows=rows, seq_len=S, max_segs=bound,
                                    row_index=rho.astype(np.int64))
        assert ref["counts"].tolist()[:2] == [rows, count]
        reached += count == bound
    assert reached >= 1
    # reached by construction: a row that starts on a document's last token, holds S - 2 one-token documents and
    # ends on the next document's first token, where no other document is shorter than 3
    assert _brute_segments(np.array([5, 1, 1, 5]), [1], 4) == ops.stream_max_segments([5, 1, 1, 5], 1, 4, True) == 4
    # the contiguous bound is unchanged by the new argument
    assert ops.stream_max_segments([3, 1, 4, 1, 5], 2, 4) == ops.stream_max_segments([3, 1, 4, 1, 5], 2, 4, False) == 6


def test_invalid_rows_and_capacity_exceeded_by_one():
    S = 4
    toks, offs = _corpus([5, 0, 9, 3, 1, 12, 4])  # T = 34: 8 full rows and a partial one
    T = int(offs[-1])
    assert T // S == 8 and T % S == 2
    good = ops.ref_stream_tokens(toks, offs, row_base=0, rows=3, seq_len=S, max_segs=12, labels=True,
                                 ignore_index=-9, row_index=np.array([6, 1, 3], dtype=np.int64))
    assert good["counts"][0] == 3
    per_row = [ops.ref_stream_tokens(toks, offs, row_base=0, rows=1, seq_len=S, max_segs=12,
                                     row_index=np.array([r], dtype=np.int64))["counts"].tolist() for r in (6, 3)]
    for bad in (-1, T // S, 1 << 40):  # negative, the partial last row, far past the end
        r = ops.ref_stream_tokens(toks, offs, row_base=0, rows=3, seq_len=S, max_segs=12, labels=True,
                                  ignore_index=-9, pad_id=3, row_index=np.array([6, bad, 3], dtype=np.int64))
        # the segment count, tokens and longest segment of the two valid rows
        assert r["counts"].tolist() == [-1, per_row[0][1] + per_row[1][1], 2 * S, max(per_row[0][3], per_row[1][3])]
        assert not r["attention_mask"].any() and not r["cu_seqlens"].any() and bool((r["labels"] == -9).all())
        assert bool((r["input_ids"] == 3).all()) and bool((r["segment_ids"] == -1).all())
        assert not r["position_ids"].any()
    n_seg = int(good["counts"][1])
    fit = ops.ref_stream_tokens(toks, offs, row_base=0, rows=3, seq_len=S, max_segs=n_seg,
                                row_index=np.array([6, 1, 3], dtype=np.int64))
    assert fit["counts"].tolist() == good["counts"].tolist() and torch.equal(fit["input_ids"], good["input_ids"])
    over = ops.ref_stream_tokens(toks, offs, row_base=0, rows=3, seq_len=S, max_segs=n_seg - 1, labels=True,
                                 row_index=np.array([6, 1, 3], dtype=np.int64))
    assert over["counts"].tolist() == [-1, *good["counts"].tolist()[1:]]  # what they would be if it fitted
    assert not over["attention_mask"].any() and not over["cu_seqlens"].any() and bool((over["labels"] == -100).all())


# ------------------------------------------------------------------- loader
@pytest.fixture(scope="module")
def source():
    src = SharedTokenSource.synthetic(f"ddl_amd_tsr_{np.random.randint(1 << 30)}", 300, 0, 90, seed=5, vocab=65536,
                                      token_dtype="uint16")
    yield src
    src.close()


GB, S = 8, 24  # 555 rows per epoch: 3 are dropped at its end


def _loader(source, rank=0, world=1, **kw):
    kw.setdefault("seed", 4)
    kw.setdefault("shuffle_rows", True)
    return ddl_amd.ResidentTokenStreamLoader(source, GB, S, DDLEnv(rank=rank, world_size=world), device="cpu", **kw)


def test_every_row_of_an_epoch_is_a_distinct_stream_row_at_every_world_size(source):
    toks, offs = source.tokens.tensor().view(-1), source.offsets.tensor().view(-1)
    dl = _loader(source, labels=True)
    n_rows = dl.order.n_samples
    assert dl.row_seed == row_seed_for(4) and 0 <= dl.row_seed < 1 << 63 and dl.row_seed != 4
    assert dl.max_segments == ops.stream_max_segments(np.diff(offs.numpy()), GB, S, shuffled_rows=True)
    assert dl.stats()["shuffle_rows"] is True and _loader(source, shuffle_rows=False).stats()["shuffle_rows"] is False
    dropped = []
    epochs = []
    for e in range(2):
        batches = list(dl)
        assert len(batches) == n_rows // GB
        order = FeistelPermutation(300, 4, e)(np.arange(300))
        stream, _ = _stream(widen_tokens(toks), offs, order)
        rho = FeistelPermutation(n_rows, row_seed_for(4), e)(np.arange(len(batches) * GB))
        assert len(set(rho.tolist())) == len(batches) * GB  # every row of the epoch is a distinct stream row
        assert not np.array_equal(rho, np.arange(rho.size))
        for g, b in enumerate(batches):
            want = np.stack([stream[r * S:(r + 1) * S] for r in rho[g * GB:(g + 1) * GB]])
            assert np.array_equal(b["input_ids"].numpy(), want), (e, g)
            assert int(b["n_rows"]) == GB and int(b["n_tokens"]) == GB * S and bool(b["attention_mask"].all())
            assert torch.equal(b["labels"], ops.ref_token_labels(b["input_ids"], b["attention_mask"],
                                                                 b["segment_ids"], -100))
        dropped.append(sorted(set(range(n_rows)) - set(rho.tolist())))
        epochs.append([b["input_ids"] for b in batches])
    # the rows dropped at the epoch's end are another set each epoch
    assert len(dropped[0]) == n_rows % GB > 0 and dropped[0] != dropped[1]
    for world in (2, 4):
        loaders = [_loader(source, r, world) for r in range(world)]
        for e in range(2):
            per_rank = [[b["input_ids"] for b in dl_r] for dl_r in loaders]
            for g, want in enumerate(epochs[e]):
                assert torch.equal(torch.cat([p[g] for p in per_rank]), want), (world, e, g)
    # shuffled rows of the unshuffled stream
    plain = next(iter(_loader(source, shuffle=False)))["input_ids"]
    stream, _ = _stream(widen_tokens(toks), offs, np.arange(300))
    rho = FeistelPermutation(n_rows, row_seed_for(4), 0)(np.arange(GB))
    assert np.array_equal(plain.numpy(), np.stack([stream[r * S:(r + 1) * S] for r in rho]))
    dl.close()


def test_checkpoints(source):
    full = [b["input_ids"] for b in _loader(source, n_epochs=1)]
    two = _loader(source, 0, 2, n_epochs=1)
    it = iter(two)
    for _ in range(3):
        next(it)
    sd = two.state_dict()
    assert sd["kind"] == "token_stream" and sd["shuffle_rows"] is True and sd["row_seed"] == row_seed_for(4)
    assert sd["global_batch_cursor"] == 3 and sd["world_size"] == 2
    # round trip mid-epoch, at the same and at another world size
    same = list(_loader(source, 0, 2, n_epochs=1, resume_state=sd))
    assert len(same) == len(full) - 3 and torch.equal(same[0]["input_ids"], full[3][:GB // 2])
    ranks = [list(_loader(source, r, 4, n_epochs=1, resume_state=sd)) for r in range(4)]
    for g in range(3, len(full)):
        assert torch.equal(torch.cat([r[g - 3]["input_ids"] for r in ranks]), full[g]), g
    # refused across shuffle_rows, in both directions; a state without the key counts as contiguous rows
    with pytest.raises(ValueError, match="shuffle_rows"):
        _loader(source, shuffle_rows=False, resume_state=sd)
    contiguous = _loader(source, shuffle_rows=False)
    sd_c = contiguous.state_dict()
    assert sd_c["shuffle_rows"] is False
    with pytest.raises(ValueError, match="shuffle_rows"):
        _loader(source, resume_state=sd_c)
    old = {k: v for k, v in sd_c.items() if k not in ("shuffle_rows", "row_seed")}
    contiguous.load_state_dict(old)
    with pytest.raises(ValueError, match="shuffle_rows"):
        _loader(source, resume_state=old)
    with pytest.raises(ValueError, match="row_seed"):
        _loader(source, resume_state=dict(sd, row_seed=1))
    # refused by and for kinds other than token_stream
    indexed = ddl_amd.ResidentTokenLoader(source, GB, S, "pack", DDLEnv(), device="cpu", seed=4)
    with pytest.raises(ValueError, match="token stream"):
        _loader(source, resume_state=indexed.state_dict())
    with pytest.raises(ValueError, match="indexed"):
        indexed.load_state_dict(sd)
    indexed.close()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_row_plan_kernel_arithmetic_under_asan_ubsan(tmp_path):
    """The per-wave loops of both launches of the row plan (csrc/kernels/tokens_stream_rows.h), replayed on the
    host over exact-size heap buffers and compared with a direct construction: a plain executable, nothing
    preloaded."""
    run_host_check(tmp_path, "tokens_stream_rows_check", "tokens stream rows check ok")
