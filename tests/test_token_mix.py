"""The weighted mix of corpus parts on the CPU: ``TokenMix`` (counts, weights, refusals), ``ops.ref_mix_order`` (how
often every document occurs, the fixed fractional subset, the written-out unshuffled order), ``order=`` of
``ops.ref_stream_tokens`` against the stream of a corpus materialised in the order, the loader's CPU twin (world
sizes, checkpoints, the trivial mix) and the host replay of the order kernel under ASan/UBSan."""

import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import TokenMix, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation, part_seed_for, row_seed_for
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "counts", "labels")


def _corpus(lens, seed=0, vocab=50000):
    lens = np.asarray(lens, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = np.random.default_rng(seed).integers(1, vocab, size=int(offs[-1]), dtype=np.int32)
    return torch.from_numpy(toks), torch.from_numpy(offs)


def materialise(toks, offs, order):
    """The epoch as a fresh corpus: tokens and offsets concatenated in ``order``."""
    o, t = offs.numpy(), toks.numpy()
    order = np.asarray(order)
    lens = o[order + 1] - o[order]
    new = np.concatenate([t[o[q]:o[q + 1]] for q in order] + [np.zeros(0, dtype=t.dtype)])
    return torch.from_numpy(new), torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


# ------------------------------------------------------------------ counts and weights
def test_counts_rounding_and_refusals():
    m = TokenMix([0, 4, 10, 14], [2.5, 1.0, 0.25])
    assert m.parts == 3 and m.n_docs == (4, 6, 4) and m.full == (2, 1, 0) and m.extra == (2, 0, 1)
    assert m.counts == (10, 6, 1) and m.cbase == (0, 10, 16, 17) and m.n_order == 17 and m.max_copies == (3, 1, 1)
    # k_p = floor(frac * n_p + 0.5): halves round up, and a fraction near 1 may take the whole part once more
    assert TokenMix([0, 2], [0.25]).extra == (1,) and TokenMix([0, 2, 3], [0.24, 1.0]).extra == (0, 0)
    assert TokenMix([0, 10], [1.96]).counts == (20,) and TokenMix([0, 10], [1.96]).max_copies == (2,)
    assert TokenMix([0, 3], [0.5]).extra == (2,) and TokenMix([0, 7], [3.0]).max_copies == (3,)
    z = TokenMix([0, 5, 9, 20], [1.0, 0.0, 2.0])  # a part that does not appear
    assert z.counts == (5, 0, 22) and z.cbase == (0, 5, 5, 27) and z.max_copies == (1, 0, 2)
    m16 = TokenMix(list(range(0, 34, 2)), [0.5 * p for p in range(16)])
    assert m16.parts == 16 and m16.n_order == sum(int(p * 0.5 * 2 + 0.5) for p in range(16)) == 120
    with pytest.raises(ValueError, match="1 to 16 parts"):
        TokenMix(list(range(18)), [1.0] * 17)
    with pytest.raises(ValueError, match="1 to 16 parts"):
        TokenMix([0], [])
    for bounds in ([0, 4, 4, 9], [0, 5, 3, 9], [1, 4, 9], [0, 4]):
        with pytest.raises(ValueError, match="bounds"):
            TokenMix(bounds, [1.0] * 3 if len(bounds) == 4 else [1.0, 1.0])
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            TokenMix([0, 4, 9], [1.0, bad])
    with pytest.raises(ValueError, match="no document"):
        TokenMix([0, 4, 9], [0.0, 0.01])
    with pytest.raises(ValueError, match="integers"):
        TokenMix([0, 4.5, 9], [1.0, 1.0])


def test_from_weights_meets_the_shares_exactly_on_uniform_parts():
    # 10 / 20 / 40 documents of 100 tokens: 1000 / 2000 / 4000 tokens; equal thirds of a 6000-token epoch
    bounds, part_tokens = [0, 10, 30, 70], [1000, 2000, 4000]
    m = TokenMix.from_weights(bounds, part_tokens, [1, 1, 1], epoch_tokens=6000)
    assert m.repeat == (2.0, 1.0, 0.5) and m.counts == (20, 20, 20)
    lens = np.full(70, 100)
    assert m.epoch_tokens(lens, seed=3) == 6000
    order = ops.ref_mix_order(m, seed=3, epoch=2)
    share = [int(lens[order[(order >= lo) & (order < hi)]].sum()) for lo, hi in zip(bounds, bounds[1:])]
    assert share == [2000, 2000, 2000]
    # the default epoch is the corpus's size; a weight of 0 drops the part, tokens or not
    d = TokenMix.from_weights(bounds, part_tokens, [1, 2, 4])
    assert d.repeat == (1.0, 1.0, 1.0)
    assert TokenMix.from_weights([0, 10, 30], [1000, 0], [3, 0]).repeat == (1.0, 0.0)
    with pytest.raises(ValueError, match="no tokens"):
        TokenMix.from_weights([0, 10, 30], [1000, 0], [1, 1])
    with pytest.raises(ValueError, match="weights"):
        TokenMix.from_weights([0, 10, 30], [1000, 10], [0, 0])
    with pytest.raises(ValueError, match="weights"):
        TokenMix.from_weights([0, 10, 30], [1000, 10], [1, -1])


# ------------------------------------------------------------------ the order
MIX = TokenMix([0, 40, 97, 98, 130, 150], [2.5, 1.0, 3.0, 0.0, 0.25])


def test_every_document_occurs_full_or_full_plus_one_times_and_the_extras_are_fixed():
    seed = 11
    orders = {e: ops.ref_mix_order(MIX, seed=seed, epoch=e) for e in (0, 1, 7)}
    extras = {}
    for e, order in orders.items():
        assert order.dtype == np.int64 and order.shape == (MIX.n_order,)
        occ = np.bincount(order, minlength=150)
        for p in range(MIX.parts):
            part = occ[MIX.bounds[p]:MIX.bounds[p + 1]]
            assert set(part.tolist()) <= {MIX.full[p], MIX.full[p] + 1}, (e, p)
            more = np.flatnonzero(part == MIX.full[p] + 1) + MIX.bounds[p]
            assert more.size == MIX.extra[p], (e, p)
            extras.setdefault(p, more)
            assert np.array_equal(extras[p], more), (e, p)  # the same documents in epochs 0, 1 and 7
            assert np.array_equal(more, np.sort(MIX.extra_documents(seed, p)))
            sigma = FeistelPermutation(MIX.n_docs[p], part_seed_for(seed, p), 0)
            assert np.array_equal(MIX.extra_documents(seed, p), MIX.bounds[p] + sigma(np.arange(MIX.extra[p])))
    assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[1], orders[7])
    assert part_seed_for(seed, 0) != part_seed_for(seed, 1) != row_seed_for(seed) and 0 <= part_seed_for(seed, 3) < 1 << 63
    # another seed: another fixed subset
    assert not np.array_equal(np.sort(MIX.extra_documents(12, 0)), extras[0])


def test_the_unshuffled_order_is_the_written_out_sequence():
    want = (list(range(0, 40)) * 2 + list(range(0, 20)) + list(range(40, 97)) + [97] * 3 + list(range(130, 135)))
    for epoch in (0, 5):
        assert ops.ref_mix_order(MIX, seed=9, epoch=epoch, shuffle=False).tolist() == want
    assert torch.equal(ops.token_mix_order(MIX, seed=9, epoch=0, shuffle=False), torch.tensor(want))
    out = torch.full((len(want) + 2,), -7, dtype=torch.int64)
    got = ops.token_mix_order(MIX, seed=9, epoch=3, out=out)
    assert got.data_ptr() == out.data_ptr() and out[-2:].tolist() == [-7, -7]
    assert np.array_equal(got.numpy(), ops.ref_mix_order(MIX, seed=9, epoch=3))
    with pytest.raises(ValueError, match="out must be"):
        ops.token_mix_order(MIX, seed=9, epoch=3, out=torch.zeros(5, dtype=torch.int64))


# ------------------------------------------------------------------ independent reference
S = 8
LENS = [0, 1, S - 1, S, S + 1, 3 * S + 2]


def _mixed_corpus(n=60, seed=1):
    rng = np.random.default_rng(seed)
    return _corpus(rng.choice(LENS, size=n), seed=seed)


@pytest.mark.parametrize("shuffle", [True, False])
def test_order_keyword_equals_the_stream_of_the_materialised_corpus(shuffle):
    toks, offs = _mixed_corpus()
    mix = TokenMix([0, 20, 21, 45, 60], [2.5, 5.0, 0.0, 0.25])
    for epoch in (0, 1):
        order = ops.ref_mix_order(mix, seed=5, epoch=epoch, shuffle=shuffle)
        mt, mo = materialise(toks, offs, order)
        T = int(mo[-1])
        assert T == mix.epoch_tokens(np.diff(offs.numpy()), 5, shuffle)
        full_rows = T // S
        rows = 5
        kw = dict(rows=rows, seq_len=S, pad_id=2, labels=True, ignore_index=-9)
        row_perm = FeistelPermutation(full_rows, 3, epoch)
        idx = np.array([full_rows - 1, 0, 3, 3, 1], dtype=np.int64)
        selections = [dict(row_base=b) for b in (0, 2, full_rows - 2, full_rows + 4)]  # the last two: past the end
        selections += [dict(row_base=0, row_perm=row_perm), dict(row_base=full_rows - rows, row_perm=row_perm),
                       dict(row_base=0, row_index=idx, max_segs=rows * S)]
        for sel in selections:
            want = ops.ref_stream_tokens(mt, mo, perm=None, **sel, **kw)
            for given in (order, torch.from_numpy(order)):
                got = ops.ref_stream_tokens(toks, offs, order=given, **sel, **kw)
                assert tuple(got) == KEYS
                for k in KEYS:
                    assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (k, sel)
            dev = ops.stream_tokens_indexed_device(toks, offs, order=torch.from_numpy(order), **sel, **kw)
            for k in KEYS:
                assert torch.equal(dev[k], want[k]), (k, sel)
    assert torch.equal(ops.token_stream_table(offs, order=torch.from_numpy(order)),
                       ops.token_stream_table(mo))


def test_neighbouring_copies_of_one_document_are_separate_segments():
    toks, offs = _corpus([3, 1, 4], seed=2)
    order = np.array([0, 1, 1, 1, 1, 1, 2], dtype=np.int64)  # a 1-token document five times over
    r = ops.ref_stream_tokens(toks, offs, order=order, row_base=0, rows=2, seq_len=8, max_segs=9)
    assert r["counts"].tolist() == [2, 7, 12, 4]  # 3 + five of 1 = row 0; the last document is cut by nothing
    assert r["cu_seqlens"].tolist() == [0, 3, 4, 5, 6, 7, 8, 12, 12, 12]
    assert r["input_ids"][0, 3:8].tolist() == [int(toks[3])] * 5 and r["position_ids"][0, 3:8].tolist() == [0] * 5
    # ids outside the corpus are empty documents
    wild = np.array([0, -1, 3, 1 << 40, 2], dtype=np.int64)
    w = ops.ref_stream_tokens(toks, offs, order=wild, row_base=0, rows=1, seq_len=8)
    assert w["counts"].tolist()[:3] == [1, 2, 7] and w["input_ids"][0, :7].tolist() == toks[[0, 1, 2, 4, 5, 6, 7]].tolist()
    with pytest.raises(ValueError, match="not both"):
        ops.ref_stream_tokens(toks, offs, order=order, perm=FeistelPermutation(3, 0, 0), row_base=0, rows=1, seq_len=8)
    with pytest.raises(TypeError, match="int64"):
        ops.ref_stream_tokens(toks, offs, order=order.astype(np.int32), row_base=0, rows=1, seq_len=8)
    with pytest.raises(ValueError, match="not both"):
        ops.token_stream_table(offs, FeistelPermutation(3, 0, 0), order=torch.from_numpy(order))


# ------------------------------------------------------------------ the loader's CPU twin
GB, SL = 4, 16
N_DOCS = 120
LMIX = TokenMix([0, 40, 41, 90, 120], [2.5, 3.0, 0.0, 0.6])


@pytest.fixture(scope="module")
def source():
    rng = np.random.default_rng(21)
    lens = rng.choice([0, 1, SL - 1, SL, SL + 1, 3 * SL + 2], size=N_DOCS)
    toks, offs = _corpus(lens, seed=21, vocab=60000)
    src = SharedTokenSource.create(f"ddl_amd_tmix_{os.getpid()}", toks.numpy(), offs.numpy(), "uint16")
    yield src
    src.close()


def _loader(source, rank=0, world=1, **kw):
    kw.setdefault("seed", 4)
    kw.setdefault("mix", LMIX)
    kw.setdefault("labels", True)
    return ddl_amd.ResidentTokenStreamLoader(source, GB, SL, DDLEnv(rank=rank, world_size=world), device="cpu", **kw)


@pytest.fixture(scope="module")
def epochs(source):
    """Three epochs at world size 1, contiguous and shuffled rows: shared by the tests below, never changed."""
    out = {}
    for shuffle_rows in (False, True):
        dl = _loader(source, shuffle_rows=shuffle_rows)
        out[shuffle_rows] = [list(dl) for _ in range(3)]
        dl.close()
    return out


@pytest.mark.parametrize("shuffle_rows", [False, True])
def test_loader_equals_the_materialised_corpus_reference(source, epochs, shuffle_rows):
    toks, offs = source.tokens.tensor().view(-1), source.offsets.tensor().view(-1)
    lens = np.diff(offs.numpy())
    dl = _loader(source, shuffle_rows=shuffle_rows)
    assert dl.n_order == LMIX.n_order and dl.stats()["mix_parts"] == 4 and dl.stats()["mix_documents"] == LMIX.n_order
    assert dl.stats()["orders_built"] == 0  # the CPU twin builds none on a device
    assert dl.max_segments == ops.stream_max_segments(np.repeat(lens, LMIX.document_copies()), GB, SL, shuffle_rows)
    tokens_of = []
    for e, batches in enumerate(epochs[shuffle_rows]):
        order = ops.ref_mix_order(LMIX, seed=4, epoch=e)
        mt, mo = materialise(toks, offs, order)
        tokens_of.append(int(mo[-1]))
        assert len(batches) == dl.batches_per_epoch == tokens_of[-1] // SL // GB > 2
        row_perm = FeistelPermutation(tokens_of[-1] // SL, row_seed_for(4), e) if shuffle_rows else None
        for g, b in enumerate(batches):
            want = ops.ref_stream_tokens(mt, mo, perm=None, row_base=g * GB, rows=GB, seq_len=SL, labels=True,
                                         max_segs=dl.max_segments, row_perm=row_perm)
            for k in KEYS[:5] + ("labels",):
                assert torch.equal(b[k], want[k]), (e, g, k)
            assert int(b["n_rows"]) == GB and int(b["n_seg"]) == int(want["counts"][1]) <= dl.max_segments
    # the epoch's token count: equal across epochs, known at construction
    assert tokens_of[0] == tokens_of[1] == tokens_of[2] == dl.total_tokens == LMIX.epoch_tokens(lens, 4)
    assert dl.total_tokens != int(lens.sum())
    assert not torch.equal(epochs[shuffle_rows][0][0]["input_ids"], epochs[shuffle_rows][1][0]["input_ids"])
    dl.close()


@pytest.mark.parametrize("world", [2, 4])
def test_union_of_the_ranks_equals_world_size_one(source, epochs, world):
    for shuffle_rows in (False, True):
        loaders = [_loader(source, r, world, shuffle_rows=shuffle_rows) for r in range(world)]
        for e in range(2):
            per_rank = [list(dl) for dl in loaders]
            for g, want in enumerate(epochs[shuffle_rows][e]):
                for k in ("input_ids", "labels", "position_ids"):
                    assert torch.equal(torch.cat([p[g][k] for p in per_rank]), want[k]), (world, e, g, k)


def test_checkpoints(source, epochs):
    full = epochs[False]
    bpe = len(full[0])
    two = _loader(source, 0, 2)
    it = iter(two)
    for _ in range(2):
        next(it)
    sd = two.state_dict()
    assert sd["mix"] == {"bounds": [0, 40, 41, 90, 120], "counts": list(LMIX.counts)} and sd["n_order"] == LMIX.n_order
    assert sd["global_batch_cursor"] == 2 and sd["total_tokens"] == two.total_tokens
    # mid-epoch, at another world size, and on across the epoch boundary
    ranks = [_loader(source, r, 4, n_epochs=2, resume_state=sd) for r in range(4)]
    rest = [list(dl) for dl in ranks]
    assert len(rest[0]) == bpe - 2
    for g in range(2, bpe):
        assert torch.equal(torch.cat([r[g - 2]["input_ids"] for r in rest]), full[0][g]["input_ids"]), g
    nxt = [list(dl) for dl in ranks]
    for g in range(bpe):
        assert torch.equal(torch.cat([r[g]["input_ids"] for r in nxt]), full[1][g]["input_ids"]), g
    # a state taken at the end of an epoch resumes at the next one
    one = _loader(source)
    assert len(list(one)) == bpe
    assert torch.equal(next(iter(_loader(source, resume_state=one.state_dict())))["input_ids"], full[1][0]["input_ids"])
    # another repeat, no mix at all, and a mix state given to a plain loader: refused
    other = TokenMix(LMIX.bounds, [2.5, 3.0, 0.0, 0.7])
    with pytest.raises(ValueError, match="mix"):
        _loader(source, mix=other, resume_state=sd)
    plain = _loader(source, mix=None)
    sd_plain = plain.state_dict()
    assert sd_plain["mix"] is None and sd_plain["n_order"] == N_DOCS
    with pytest.raises(ValueError, match="mix"):
        _loader(source, resume_state=sd_plain)
    with pytest.raises(ValueError, match="mix"):
        _loader(source, mix=None, resume_state=sd)
    old = {k: v for k, v in sd_plain.items() if k not in ("mix", "n_order")}  # a state from before the key existed
    plain.load_state_dict(old)
    with pytest.raises(ValueError, match="mix"):
        _loader(source, resume_state=old)
    with pytest.raises(ValueError, match="documents"):
        _loader(source, mix=TokenMix([0, 100], [1.0]))
    with pytest.raises(TypeError, match="TokenMix"):
        _loader(source, mix=[1.0])


@pytest.mark.parametrize("shuffle", [True, False])
def test_the_trivial_mix_equals_no_mix(source, shuffle):
    for shuffle_rows in (False, True):
        a = _loader(source, mix=TokenMix([0, N_DOCS], [1.0]), shuffle=shuffle, shuffle_rows=shuffle_rows)
        b = _loader(source, mix=None, shuffle=shuffle, shuffle_rows=shuffle_rows)
        assert a.total_tokens == b.total_tokens and a.max_segments == b.max_segments
        for e in range(2):
            xs, ys = list(a), list(b)
            assert len(xs) == len(ys) > 0
            for x, y in zip(xs, ys):
                assert list(x) == list(y)
                for k in y:
                    assert torch.equal(x[k], y[k]) if isinstance(y[k], torch.Tensor) else x[k] == y[k], (e, k)


# ------------------------------------------------------------------ host check and example
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_order_kernel_arithmetic_under_asan_ubsan(tmp_path):
    """The per-lane routine of ``token_mix_order`` (csrc/kernels/tokens_mix.h), replayed on the host for every
    entry over index-checked views and compared with an order written out independently: a plain executable,
    nothing preloaded."""
    run_host_check(tmp_path, "tokens_mix_check", "tokens mix check ok")


def test_example_with_a_mix_on_the_cpu():
    env = dict(os.environ, DDL_DEVICE="cpu", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "tokens_packed.py"), "--resident", "--stream",
                        "--mix", "2,1,0.5", "--n-seqs", "96", "--seq-len", "256", "--global-batch", "4", "--epochs",
                        "2"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "mix: 3 parts x [2.0, 1.0, 0.5] -> 112 documents" in r.stdout
    assert r.stdout.count("100.0% dense") == 2
