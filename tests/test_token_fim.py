"""Fill-in-the-middle rearrangement on the CPU: ``TokenFIM`` (quantisation, refusals), ``ops.ref_fim_tokens`` against
a per-segment reference kept here (Python lists and slicing, ``mix64`` in Python integers: no code shared with the
op), its properties and selection rates, the loaders' CPU twin (world sizes, shuffled rows, a mix, checkpoints), the
host replay of the kernel's lane routine under ASan/UBSan and the example."""

import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import TokenFIM, TokenMix, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation, fim_seed_for, row_seed_for
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
PRE, MID, SUF, EOD = 70001, 70002, 70003, 49999  # sentinels past a uint16 vocabulary; EOD inside it
VOCAB = 49999  # corpus tokens are drawn from [1, VOCAB): none is a sentinel or the EOD


# ------------------------------------------------------------------ the test's own reference
def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def epoch_key(seed, epoch):
    fim_seed = mix64(seed ^ 0x66696D5F63757473) & ((1 << 63) - 1)
    return mix64((fim_seed + (epoch + 1) * 0x9E3779B97F4A7C15) & M64)


def my_segment(t, key, ekey, rate_q, spm_q, min_len, eod):
    """(new tokens, kind) of one segment ``t`` (a list): kind None = not eligible, "keep", "psm" or "spm"."""
    u = [mix64(ekey ^ mix64((4 * (key & M64) + c) & M64)) for c in range(4)]
    tail = 1 if eod is not None and t[-1] == eod else 0
    body = t[:len(t) - tail]
    if len(body) < min_len:
        return list(t), None
    if not (u[0] >> 40) < rate_q:
        return list(t), "keep"
    K = len(body) - 3
    x, y = ((u[2] >> 32) * (K + 1)) >> 32, ((u[3] >> 32) * (K + 1)) >> 32
    a, b = min(x, y), max(x, y)
    pre, mid, suf = body[:a], body[a:b], body[b:K]
    if (u[1] >> 40) < spm_q:
        new, kind = [PRE, SUF] + suf + [MID] + pre + mid, "spm"
    else:
        new, kind = [PRE] + pre + [SUF] + suf + [MID] + mid, "psm"
    return new + t[len(body):], kind


def segments_of(batch):
    """(row, first column, length) of every segment, from the segment ids alone, in segment order."""
    out = []
    for r, row in enumerate(batch["segment_ids"].tolist()):
        c = 0
        while c < len(row):
            e = c
            while e < len(row) and row[e] == row[c]:
                e += 1
            if row[c] >= 0:
                out.append((r, c, e - c))
            c = e
    return out


def my_fim(batch, keys, seed, epoch, *, rate, spm_rate=0.5, min_len=8, eod=None):
    """(the rearranged ids as a tensor, the kind of every segment)."""
    ids = [list(r) for r in batch["input_ids"].tolist()]
    kinds = []
    live = int(batch["counts"][0] if "counts" in batch else batch.get("n_rows", 0)) >= 0
    for s, (r, c, n) in enumerate(segments_of(batch)):
        new, kind = my_segment(ids[r][c:c + n], int(keys[s]), epoch_key(seed, epoch), round(rate * 2 ** 24),
                               round(spm_rate * 2 ** 24), min_len, eod) if live else (ids[r][c:c + n], None)
        assert len(new) == n
        ids[r][c:c + n] = new
        kinds.append(kind)
    return torch.tensor(ids, dtype=torch.int32), kinds


def stream_elements(offs, order):
    """The corpus element of every token of the stream of documents ``order``."""
    o = np.asarray(offs)
    return np.concatenate([np.arange(o[q], o[q + 1], dtype=np.int64) for q in order] + [np.zeros(0, dtype=np.int64)])


def my_keys(batch, elems, stream_rows, S):
    """The key of every segment of a batch whose row ``k`` is stream row ``stream_rows[k]``: the corpus element of
    the segment's first token."""
    return [int(elems[stream_rows[r] * S + c]) for r, c, _ in segments_of(batch)]


def _corpus(lens, seed, eod=None, mid_doc=None):
    lens = np.asarray(lens, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = np.random.default_rng(seed).integers(1, VOCAB, size=int(offs[-1]), dtype=np.int32)
    if eod is not None:
        toks[offs[1:][lens > 0] - 1] = eod  # every document ends in the EOD
        if mid_doc is not None:
            toks[(offs[mid_doc] + offs[mid_doc + 1]) // 2] = eod  # and one holds it mid-way
    return torch.from_numpy(toks), torch.from_numpy(offs)


def grid_lens(S):
    """Documents of every length of the grid; the long ones first and aligned, so that full-row pieces exist."""
    return [3 * S + 2, S - 2, 0, 1, 3, 4, 5, S - 1, S, S + 1, 3 * S + 2, S, 4, S + 1, 5, S - 1, 1, 0, 3, 3 * S + 2, S, S]


def grid_batches(S, eod):
    """Two batches of 5 rows of the unshuffled stream over ``grid_lens``, with their keys."""
    toks, offs = _corpus(grid_lens(S), seed=S, eod=eod, mid_doc=10)
    elems = stream_elements(offs, range(len(offs) - 1))
    out = []
    for base in (0, 5):
        b = ops.ref_stream_tokens(toks, offs, row_base=base, rows=5, seq_len=S)
        out.append((b, my_keys(b, elems, list(range(base, base + 5)), S)))
    return out


# seeds at which, at rate 0.5, the two batches of a (S, eod, min_len) case hold a rearranged and an untouched
# eligible segment between them (searched once; the test asserts it)
GRID_SEED = {(8, False, 4): 0, (8, False, 8): 0, (8, True, 4): 0, (8, True, 8): 0, (10, False, 4): 0,
             (10, False, 8): 0, (10, True, 4): 0, (10, True, 8): 1, (516, False, 4): 0, (516, False, 8): 0,
             (516, True, 4): 0, (516, True, 8): 0}


# ------------------------------------------------------------------ the specification
def test_spec_quantises_once_and_refuses_bad_values():
    f = TokenFIM(0.5, prefix_id=PRE, middle_id=MID, suffix_id=SUF)
    assert f.rate_q == 1 << 23 and f.spm_q == 1 << 23 and f.min_len == 8 and f.eod_id is None
    assert TokenFIM(0.9, prefix_id=1, middle_id=2, suffix_id=3).rate_q == round(0.9 * 2 ** 24)
    assert TokenFIM(1, prefix_id=1, middle_id=2, suffix_id=3, spm_rate=0).state() == {
        "rate_q": 1 << 24, "spm_q": 0, "prefix_id": 1, "middle_id": 2, "suffix_id": 3, "eod_id": None, "min_len": 8}
    assert f.epoch_key(7, 3) == epoch_key(7, 3) and fim_seed_for(7) != row_seed_for(7) and 0 <= fim_seed_for(7) < 1 << 63
    ok = dict(prefix_id=1, middle_id=2, suffix_id=3)
    for name, bad in (("rate", -0.1), ("rate", 1.5), ("rate", float("nan")), ("rate", "x")):
        with pytest.raises(ValueError, match=name):
            TokenFIM(bad, **ok)
    with pytest.raises(ValueError, match="spm_rate"):
        TokenFIM(0.5, spm_rate=2, **ok)
    for name in ("prefix_id", "middle_id", "suffix_id", "eod_id"):
        for bad in (1 << 31, -(1 << 31) - 1, 1.5, "a"):
            with pytest.raises(ValueError, match=name):
                TokenFIM(0.5, **{**ok, name: bad})
    with pytest.raises(ValueError, match="min_len"):
        TokenFIM(0.5, min_len=3, **ok)
    with pytest.raises(TypeError, match="TokenFIM"):
        ops.ref_fim_tokens({}, 0.5, seg_keys=[], seed=0, epoch=0)


# ------------------------------------------------------------------ the op against the test's reference
@pytest.mark.parametrize("eod", [None, EOD])
@pytest.mark.parametrize("S", [8, 10, 516])
def test_ref_equals_the_per_segment_reference(S, eod):
    batches = grid_batches(S, eod)
    for min_len in (4, 8):
        seed = GRID_SEED[(S, eod is not None, min_len)]
        for rate in (0, 0.5, 1):
            for spm_rate in (0, 0.5, 1):
                fim = TokenFIM(rate, prefix_id=PRE, middle_id=MID, suffix_id=SUF, spm_rate=spm_rate, eod_id=eod,
                               min_len=min_len)
                all_kinds = []  # of the case's two batches
                for n, (b, keys) in enumerate(batches):
                    case = (S, eod, min_len, rate, spm_rate, n)
                    want, kinds = my_fim(b, keys, seed, 3, rate=rate, spm_rate=spm_rate, min_len=min_len, eod=eod)
                    got = ops.ref_fim_tokens(b, fim, seg_keys=np.asarray(keys, dtype=np.int64), seed=seed, epoch=3,
                                             labels=True)
                    assert got["input_ids"].dtype == torch.int32 and torch.equal(got["input_ids"], want), case
                    assert torch.equal(got["labels"], ops.ref_token_labels(want, b["attention_mask"],
                                                                           b["segment_ids"])), case
                    for k in b:  # every other entry is the input's own
                        assert k == "input_ids" or got[k] is b[k], (case, k)
                    assert torch.equal(ops.fim_tokens(b, fim, seg_keys=torch.tensor(keys), seed=seed,
                                                      epoch=3)["input_ids"], want), case  # CPU tensors: the reference
                    all_kinds += kinds
                    if rate == 0:
                        assert torch.equal(got["input_ids"], b["input_ids"]), case
                case = case[:-1]
                moved = [k for k in all_kinds if k in ("psm", "spm")]
                assert None in all_kinds, case  # bodies below min_len stay as they are
                if rate == 0.5:  # a rearranged and an untouched eligible segment
                    assert moved and "keep" in all_kinds, case
                if rate == 0:
                    assert not moved and "keep" in all_kinds, case
                if rate == 1:
                    assert "keep" not in all_kinds and moved, case
                    if spm_rate in (0, 1):
                        assert set(moved) == {"spm" if spm_rate else "psm"}, case


def test_properties_of_a_rearranged_segment():
    S, eod = 516, EOD
    fim = TokenFIM(1.0, prefix_id=PRE, middle_id=MID, suffix_id=SUF, eod_id=eod, min_len=4)
    seen = set()
    for b, keys in grid_batches(S, eod):
        for epoch in range(4):
            got = ops.ref_fim_tokens(b, fim, seg_keys=np.asarray(keys), seed=1, epoch=epoch)["input_ids"].tolist()
            for (r, c, n) in segments_of(b):
                t, new = b["input_ids"][r, c:c + n].tolist(), got[r][c:c + n]
                tail = 1 if t[-1] == eod else 0
                if n - tail < 4:
                    assert new == t
                    continue
                K = n - tail - 3
                assert sum(new.count(x) for x in (PRE, MID, SUF)) == 3 and new[0] == PRE
                assert new[n - tail:] == t[n - tail:]  # the EOD stays last
                body = new[:n - tail]
                rest = [x for x in body if x not in (PRE, MID, SUF)]
                assert sorted(rest) == sorted(t[:K])
                i_suf, i_mid = body.index(SUF), body.index(MID)
                assert i_suf < i_mid
                # PSM: [PRE] pre [SUF] suf [MID] mid; SPM: [PRE] [SUF] suf [MID] pre mid (pre is empty between)
                undone = body[1:i_suf] + body[i_mid + 1:] + body[i_suf + 1:i_mid]
                assert undone == t[:K]
                seen.add("spm" if i_suf == 1 else "psm")
    assert seen == {"spm", "psm"}


def test_an_overflowed_batch_and_unsound_segments_are_left_alone():
    toks, offs = _corpus(grid_lens(8), seed=1)
    fim = TokenFIM(1.0, prefix_id=PRE, middle_id=MID, suffix_id=SUF, min_len=4)
    over = ops.ref_stream_tokens(toks, offs, row_base=0, rows=5, seq_len=8, max_segs=2, labels=True)
    assert int(over["counts"][0]) == -1
    got = ops.ref_fim_tokens(over, fim, seg_keys=np.zeros(2, dtype=np.int64), seed=0, epoch=0, labels=True)
    assert torch.equal(got["input_ids"], over["input_ids"]) and torch.equal(got["labels"], over["labels"])
    # n_rows = -1 on a batch that does hold segments (the loaders' key), segment ids past the keys, a run that
    # claims more tokens than its row holds: nothing is rearranged, nothing outside the tensors is read
    b = ops.ref_stream_tokens(toks, offs, row_base=0, rows=5, seq_len=8)
    keys = np.arange(int(b["counts"][1]), dtype=np.int64)
    assert not torch.equal(ops.ref_fim_tokens(b, fim, seg_keys=keys, seed=0, epoch=0)["input_ids"], b["input_ids"])
    dead = {k: v for k, v in b.items() if k != "counts"}
    dead["n_rows"] = torch.tensor(-1)
    assert torch.equal(ops.ref_fim_tokens(dead, fim, seg_keys=keys, seed=0, epoch=0)["input_ids"], b["input_ids"])
    assert torch.equal(ops.ref_fim_tokens(b, fim, seg_keys=keys[:0], seed=0, epoch=0)["input_ids"], b["input_ids"])
    wild = dict(b, cu_seqlens=torch.arange(0, 100 * b["cu_seqlens"].numel(), 100, dtype=torch.int32))
    assert torch.equal(ops.ref_fim_tokens(wild, fim, seg_keys=keys, seed=0, epoch=0)["input_ids"], b["input_ids"])
    wild = dict(b, segment_ids=b["segment_ids"] + 1000, position_ids=b["position_ids"] - 3)
    assert torch.equal(ops.ref_fim_tokens(wild, fim, seg_keys=keys, seed=0, epoch=0)["input_ids"], b["input_ids"])


@pytest.mark.parametrize("rate,spm_rate", [(0.5, 0.5), (0.9, 0.25)])
def test_selection_and_variant_rates(rate, spm_rate):
    R, S, n = 2100, 16, 4200  # two segments of 8 tokens per row, every one eligible
    ids = torch.from_numpy(np.random.default_rng(5).integers(1, VOCAB, size=(R, S), dtype=np.int32))
    batch = {"input_ids": ids, "attention_mask": torch.ones(R, S, dtype=torch.uint8),
             "position_ids": torch.arange(8).repeat(R, 2), "segment_ids": torch.arange(n, dtype=torch.int32).view(R, 2)
             .repeat_interleave(8, dim=1), "cu_seqlens": torch.arange(0, 8 * n + 1, 8, dtype=torch.int32)}
    fim = TokenFIM(rate, prefix_id=PRE, middle_id=MID, suffix_id=SUF, spm_rate=spm_rate)
    keys = np.random.default_rng(6).integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64)
    want, kinds = my_fim(batch, keys, 9, 0, rate=rate, spm_rate=spm_rate)
    out = ops.ref_fim_tokens(batch, fim, seg_keys=keys, seed=9, epoch=0)["input_ids"]
    assert torch.equal(out, want)
    heads = out.view(n, 8)
    moved = heads[:, 0] == PRE
    spm = heads[:, 1] == SUF  # PSM with an empty prefix looks the same: count the kinds of the reference instead
    n_moved = int(moved.sum())
    assert n_moved == sum(k in ("psm", "spm") for k in kinds) and bool((spm <= moved).all())
    assert abs(n_moved / n - fim.rate_q / 2 ** 24) <= 5 * math.sqrt(rate * (1 - rate) / n)
    n_spm = kinds.count("spm")
    assert abs(n_spm / n_moved - fim.spm_q / 2 ** 24) <= 5 * math.sqrt(spm_rate * (1 - spm_rate) / n_moved)


# ------------------------------------------------------------------ the loader's CPU twin
GB, SL, N_DOCS, SEED = 4, 16, 120, 4
FIM = TokenFIM(0.5, prefix_id=PRE, middle_id=MID, suffix_id=SUF, eod_id=EOD, min_len=4)
LMIX = TokenMix([0, 40, 41, 90, 120], [2.5, 3.0, 0.0, 0.6])


@pytest.fixture(scope="module")
def source():
    lens = np.random.default_rng(21).choice([0, 1, 3, 4, 5, SL - 1, SL, SL + 1, 3 * SL + 2], size=N_DOCS)
    toks, offs = _corpus(lens, seed=21, eod=EOD, mid_doc=int(np.argmax(lens)))
    src = SharedTokenSource.create(f"ddl_amd_tfim_{os.getpid()}", toks.numpy(), offs.numpy(), "uint16")
    yield src
    src.close()


def _loader(source, rank=0, world=1, **kw):
    kw.setdefault("seed", SEED)
    kw.setdefault("fim", FIM)
    kw.setdefault("labels", True)
    return ddl_amd.ResidentTokenStreamLoader(source, GB, SL, DDLEnv(rank=rank, world_size=world), device="cpu", **kw)


CONFIGS = [dict(), dict(shuffle_rows=True), dict(labels=False), dict(mix=LMIX), dict(mix=LMIX, shuffle_rows=True)]


def _cfg_id(cfg):
    return ",".join(f"{k}={'mix' if k == 'mix' else v}" for k, v in cfg.items()) or "plain"


@pytest.fixture(scope="module")
def epochs(source):
    """Two epochs at world size 1 of every configuration: shared by the tests below, never changed."""
    out = {}
    for cfg in CONFIGS:
        dl = _loader(source, **cfg)
        out[_cfg_id(cfg)] = [list(dl) for _ in range(2)]
        dl.close()
    return out


@pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)
def test_loader_equals_the_stream_reference_and_the_tests_rearrangement(source, epochs, cfg):
    toks, offs = source.tokens.tensor().view(-1), source.offsets.tensor().view(-1)
    dl = _loader(source, **cfg)
    assert dl.stats()["fim"] is True and dl.state_dict()["fim"] == FIM.state()
    labels, mix, shuffle_rows = cfg.get("labels", True), cfg.get("mix"), cfg.get("shuffle_rows", False)
    n_moved = n_kept = 0
    for e, batches in enumerate(epochs[_cfg_id(cfg)]):
        order = (ops.ref_mix_order(mix, seed=SEED, epoch=e) if mix is not None
                 else FeistelPermutation(N_DOCS, SEED, e)(np.arange(N_DOCS)))
        elems = stream_elements(offs.numpy(), order)
        row_perm = FeistelPermutation(dl.order.n_samples, row_seed_for(SEED), e) if shuffle_rows else None
        assert len(batches) == dl.batches_per_epoch > 2
        for g, b in enumerate(batches):
            plain = ops.ref_stream_tokens(toks, offs, order=order, row_base=g * GB, rows=GB, seq_len=SL,
                                          max_segs=dl.max_segments, row_perm=row_perm)
            rows = np.arange(g * GB, (g + 1) * GB)
            rows = row_perm(rows) if shuffle_rows else rows
            want, kinds = my_fim(plain, my_keys(plain, elems, rows.tolist(), SL), SEED, e, rate=0.5, min_len=4, eod=EOD)
            assert torch.equal(b["input_ids"], want), (e, g)
            assert ("labels" in b) == labels
            if labels:
                assert torch.equal(b["labels"], ops.ref_token_labels(want, plain["attention_mask"], plain["segment_ids"]))
            for k in ("attention_mask", "position_ids", "segment_ids", "cu_seqlens"):
                assert torch.equal(b[k], plain[k]), (e, g, k)
            assert int(b["n_rows"]) == GB and int(b["n_seg"]) == int(plain["counts"][1])
            n_moved += sum(k in ("psm", "spm") for k in kinds)
            n_kept += kinds.count("keep")
    assert n_moved > 10 and n_kept > 10
    dl.close()


@pytest.mark.parametrize("world", [2, 4])
def test_union_of_the_ranks_equals_world_size_one(source, epochs, world):
    for cfg in (dict(), dict(shuffle_rows=True), dict(mix=LMIX)):
        loaders = [_loader(source, r, world, **cfg) for r in range(world)]
        for e in range(2):
            per_rank = [list(dl) for dl in loaders]
            for g, want in enumerate(epochs[_cfg_id(cfg)][e]):
                for k in ("input_ids", "labels"):
                    assert torch.equal(torch.cat([p[g][k] for p in per_rank]), want[k]), (world, e, g, k)
        for dl in loaders:
            dl.close()


@pytest.mark.parametrize("mix", [None, LMIX], ids=["plain", "mix"])
def test_a_shuffled_row_equals_the_same_stream_row_of_the_contiguous_epoch(source, epochs, mix):
    base = dict() if mix is None else dict(mix=mix)
    dl = _loader(source, shuffle_rows=True, **base)
    checked = 0
    for e in range(2):
        flat = {k: torch.cat([b[k] for b in epochs[_cfg_id(base)][e]]) for k in ("input_ids", "labels")}
        rho = FeistelPermutation(dl.order.n_samples, row_seed_for(SEED), e)
        for g, b in enumerate(epochs[_cfg_id(dict(base, shuffle_rows=True))][e]):
            for j, r in enumerate(rho(np.arange(g * GB, (g + 1) * GB)).tolist()):
                if r < flat["input_ids"].shape[0]:  # the contiguous epoch drops its last rows
                    assert torch.equal(b["input_ids"][j], flat["input_ids"][r]), (e, g, j)
                    assert torch.equal(b["labels"][j], flat["labels"][r]), (e, g, j)
                    checked += 1
    assert checked > 20
    dl.close()


def test_two_epochs_of_the_same_rows_are_rearranged_differently(source):
    dl, plain = _loader(source, shuffle=False), _loader(source, shuffle=False, fim=None)
    e0, e1, p0 = list(dl), list(dl), list(plain)
    assert len(e0) == len(e1) == len(p0) > 2
    assert any(not torch.equal(a["input_ids"], b["input_ids"]) for a, b in zip(e0, e1))
    assert any(not torch.equal(a["input_ids"], b["input_ids"]) for a, b in zip(e0, p0))
    for a, b, p in zip(e0, e1, p0):  # the same rows: only the arrangement inside the segments differs
        assert torch.equal(a["segment_ids"], b["segment_ids"]) and torch.equal(a["cu_seqlens"], p["cu_seqlens"])
    dl.close()
    plain.close()


def test_checkpoints(source, epochs):
    full = epochs["plain"]
    bpe = len(full[0])
    two = _loader(source, 0, 2)
    it = iter(two)
    for _ in range(2):
        next(it)
    sd = two.state_dict()
    assert sd["fim"] == FIM.state() and sd["global_batch_cursor"] == 2
    ranks = [_loader(source, r, 4, n_epochs=2, resume_state=sd) for r in range(4)]  # mid-epoch, another world size
    rest = [list(dl) for dl in ranks]
    assert len(rest[0]) == bpe - 2
    for g in range(2, bpe):
        for k in ("input_ids", "labels"):
            assert torch.equal(torch.cat([r[g - 2][k] for r in rest]), full[0][g][k]), (g, k)
    nxt = [list(dl) for dl in ranks]
    for g in range(bpe):
        assert torch.equal(torch.cat([r[g]["input_ids"] for r in nxt]), full[1][g]["input_ids"]), g
    # another specification, none where one was saved, one where none was saved: refused
    other = TokenFIM(0.25, prefix_id=PRE, middle_id=MID, suffix_id=SUF, eod_id=EOD, min_len=4)
    with pytest.raises(ValueError, match="fim"):
        _loader(source, fim=other, resume_state=sd)
    with pytest.raises(ValueError, match="fim"):
        _loader(source, fim=None, resume_state=sd)
    plain = _loader(source, fim=None)
    sd_plain = plain.state_dict()
    assert sd_plain["fim"] is None and plain.stats()["fim"] is False
    with pytest.raises(ValueError, match="fim"):
        _loader(source, resume_state=sd_plain)
    old = {k: v for k, v in sd_plain.items() if k != "fim"}  # a state from before the key existed: no FIM
    plain.load_state_dict(old)
    with pytest.raises(ValueError, match="fim"):
        _loader(source, resume_state=old)
    with pytest.raises(TypeError, match="TokenFIM"):
        _loader(source, fim=0.5)
    for dl in [two, plain] + ranks:
        dl.close()


def test_without_fim_the_batches_are_the_stream_reference(source):
    toks, offs = source.tokens.tensor().view(-1), source.offsets.tensor().view(-1)
    dl = _loader(source, fim=None, shuffle_rows=True)
    for g, b in enumerate(dl):
        want = ops.ref_stream_tokens(toks, offs, perm=FeistelPermutation(N_DOCS, SEED, 0), row_base=g * GB, rows=GB,
                                     seq_len=SL, max_segs=dl.max_segments, labels=True,
                                     row_perm=FeistelPermutation(dl.order.n_samples, row_seed_for(SEED), 0))
        assert list(b) == ["input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "labels",
                           "max_seqlen", "n_tokens", "n_rows", "n_seg"]
        for k in ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "labels"):
            assert torch.equal(b[k], want[k]), (g, k)
    with_fim = _loader(source)
    assert list(next(iter(with_fim))) == list(b)  # and FIM adds no key
    with_fim.close()
    dl.close()


# ------------------------------------------------------------------ host check and example
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_lane_routine_under_asan_ubsan(tmp_path):
    """The per-lane routine of ``token_fim`` (csrc/kernels/tokens_fim.h), replayed on the host for every lane of
    every workgroup over exact-size, index-checked buffers and compared with layouts written out independently: a
    plain executable, nothing preloaded."""
    run_host_check(tmp_path, "tokens_fim_check", "tokens fim check ok")


def test_example_with_fim_on_the_cpu():
    env = dict(os.environ, DDL_DEVICE="cpu", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "tokens_packed.py"), "--resident", "--stream",
                        "--fim", "0.5", "--n-seqs", "96", "--seq-len", "256", "--global-batch", "4", "--epochs", "1"],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("fim:")]
    assert len(line) == 1 and "segments rearranged" in line[0], r.stdout[-2000:]
