"""The batch descriptor kernel against NumPy, the device-planned indexed ops against their CPU reference path
(bitwise), and ``ResidentTokenLoader(plan="device")`` against its CPU twin and against the host plan."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import _native, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.ops.kernels import _index_kw, segment_sources
from ddl_amd.permutation import EpochOrder, FeistelPermutation
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GB = 16
GUARD = 64
SENTINEL = 0x5A
SENTINEL64 = int.from_bytes(bytes([SENTINEL]) * 8, "little")


def _guarded(need):
    full = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert full.data_ptr() % 16 == 0
    return full, full[GUARD:GUARD + need]


def _check_guards(full, need):
    host = full.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + need:] == SENTINEL).all())


# --------------------------------------------------------------- descriptor
def _lens_corpus(n_corpus, mod):
    """Corpus offsets of sequences of lengths i % mod (every mod-th one is empty)."""
    lens = np.arange(n_corpus) % mod
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _descriptor_and_plan(coffs_dev, n_corpus, selector, n, S, max_segs, max_rows):
    """token_batch_descriptor + pack_plan_device, as the op launches them, into one sentinel-filled buffer
    inside guard bytes. Returns the arrays on the host."""
    h = _native.hip()
    sizes = [8 * n, 8 * (n + 1), 8 * max_segs, 8 * (max_segs + 1), 8 * max_rows, 8 * max_rows, 32,
             4 * h.pack_plan_scratch_ints(max_segs, max_rows)]
    starts = np.concatenate([[0], np.cumsum([-(-b // 16) * 16 for b in sizes])])
    need = int(starts[-1])
    full, buf = _guarded(need)
    p = [buf.data_ptr() + int(s) for s in starts[:-1]]
    sh = torch.cuda.current_stream().cuda_stream
    h.token_batch_descriptor(corpus_offsets=coffs_dev.data_ptr(), n_corpus=n_corpus, n=n, seq_len=S,
                             max_segs=max_segs, src_start=p[0], offsets=p[1], seg_src=p[2], counts=p[6],
                             pad_counts=False, stream=sh, **selector)
    h.pack_plan_device(offsets=p[1], n=n, seq_len=S, max_segs=max_segs, max_rows=max_rows, seg_offsets=p[3],
                       row_start=p[4], row_end=p[5], counts=p[6], scratch=p[7], stream=sh)
    torch.cuda.synchronize()
    _check_guards(full, need)
    host = buf.cpu().numpy()
    names = ("src_start", "offsets", "seg_src", "seg_offsets", "row_start", "row_end", "counts")
    return {k: host[int(starts[i]):int(starts[i]) + sizes[i]].view(np.int64) for i, k in enumerate(names)}


def _check_descriptor(coffs, idx, selector_of, S):
    """The kernels' arrays for the sequences ``idx`` against NumPy, bit for bit, for every given selector."""
    n, n_corpus = len(idx), len(coffs) - 1
    src_start = coffs[idx]
    lens = coffs[idx + 1] - src_start
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rs, re_, so = ops.ref_pack_plan(offsets, S)
    n_seg = len(so) - 1
    seg_src = segment_sources(src_start, offsets, so, n_seg)
    max_segs, max_rows = n_seg + 3, len(rs) + 2
    coffs_dev = torch.from_numpy(coffs).cuda()
    results = []
    for make in selector_of:
        keep, selector = make()
        got = _descriptor_and_plan(coffs_dev, n_corpus, selector, n, S, max_segs, max_rows)
        del keep
        assert np.array_equal(got["src_start"], src_start)
        assert np.array_equal(got["offsets"], offsets)
        assert np.array_equal(got["seg_src"][:n_seg], seg_src)
        assert (got["seg_src"][n_seg:] == SENTINEL64).all()  # nothing past the batch's segments
        assert np.array_equal(got["seg_offsets"][:n_seg + 1], so)
        assert np.array_equal(got["row_start"][:len(rs)], rs) and np.array_equal(got["row_end"][:len(rs)], re_)
        max_seg = int(min(lens.max(), S)) if n else 0
        assert got["counts"].tolist() == [len(rs), n_seg, int(offsets[-1]), max_seg]
        results.append(got)
    return results


def _feistel(perm, base):
    return lambda: (None, _index_kw(None, perm, base))


def _explicit(idx):
    def make():
        t = torch.from_numpy(np.ascontiguousarray(idx)).cuda()
        return t, _index_kw(t, None, 0)
    return make


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_descriptor_matches_numpy_at_wave_and_tile_edges(n):
    """A Feistel domain of 3001 sequences (no power of two: cycle walking runs), lengths i % 13 (empty sequences
    in every tile), base > 0, and the explicit index of the same positions."""
    coffs = _lens_corpus(3001, 13)
    perm = FeistelPermutation(3001, seed=11, epoch=2)
    base = min(n, 3001 - n)
    idx = perm(np.arange(base, base + n, dtype=np.int64))
    assert len(set(idx.tolist())) == n and idx.max() < 3001
    a, b = _check_descriptor(coffs, idx, [_feistel(perm, base), _explicit(idx)], 37)
    for k in ("src_start", "offsets", "counts"):
        assert np.array_equal(a[k], b[k])


def test_descriptor_of_a_late_rank_1_batch_of_the_epoch_order():
    order = EpochOrder(1100, 128, seed=5)
    e, g, rank, world = 3, 7, 1, 2
    idx = np.asarray(order.indices(e, g, rank, world), dtype=np.int64)
    base = g * 128 + rank * 64
    _check_descriptor(_lens_corpus(1100, 13), idx, [_feistel(order.perm(e), base)], 37)
    ident = np.arange(base, base + 64, dtype=np.int64)  # shuffle=False: the identity selector
    _check_descriptor(_lens_corpus(1100, 13), ident, [lambda: (None, _index_kw(None, None, base))], 37)


def test_descriptor_splits_long_sequences_into_segments():
    """seq_len 6 with lengths up to 40: up to 7 segments per sequence, seg_src takes its j * S terms."""
    coffs = _lens_corpus(3001, 41)
    perm = FeistelPermutation(3001, seed=1, epoch=0)
    idx = perm(np.arange(100, 100 + 1025, dtype=np.int64))
    (got,) = _check_descriptor(coffs, idx, [_feistel(perm, 100)], 6)
    assert got["counts"][1] > 2 * 1025 and got["counts"][3] == 6


def test_descriptor_of_an_all_empty_batch():
    coffs = _lens_corpus(3001, 13)
    idx = (np.arange(100, dtype=np.int64) * 13) % 3001 // 13 * 13
    assert (coffs[idx + 1] - coffs[idx] == 0).all()
    (got,) = _check_descriptor(coffs, idx, [_explicit(idx)], 37)
    assert got["counts"].tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------- ops
WANTED = [0, 1, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1000, 0, 5]


def _ragged_corpus(np_dtype):
    """(tokens, offsets, idx): the wanted sequences with fillers between them so that wanted sequence i starts at
    residue i % 8 (elements); idx also holds a repeated index and the corpus's first and last sequence."""
    lens, idx, at = [6], [], 6
    for i, n in enumerate(WANTED):
        fill = (i - at) % 8
        lens += [fill, n]
        idx.append(len(lens) - 1)
        at += fill + n
    lens.append(11)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx += [0, len(lens) - 1, idx[9], idx[12]]
    info = np.iinfo(np_dtype)
    toks = np.random.default_rng(5).integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True)
    return toks, offs, np.asarray(idx, dtype=np.int64)


def _same_dict(got, ref):
    assert list(got) == list(ref)
    for k in ref:
        a, b = got[k], ref[k]
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b), k


def _check_device_ops(toks, offs, sel_cpu, seq_len, pdt=torch.int64, pad_id=-3, caps=None):
    """Both device-planned ops, with and without ``out=`` (a slice of a sentinel-filled buffer inside guard
    bytes), bitwise against the same ops on CPU tensors (their reference path). Returns the pack reference."""
    caps = caps or {}
    t_cpu, o_cpu = torch.from_numpy(toks), torch.from_numpy(offs)
    corpus, coffs = t_cpu.cuda(), o_cpu.cuda()
    sel = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in sel_cpu.items()}
    kw = dict(seq_len=seq_len, pad_id=pad_id, position_dtype=pdt)
    pad_ref = ops.pad_tokens_indexed_device(t_cpu, o_cpu, **sel_cpu, **kw)
    pack_ref = ops.pack_tokens_indexed_device(t_cpu, o_cpu, **sel_cpu, **kw, **caps)
    _same_dict(ops.pad_tokens_indexed_device(corpus, coffs, **sel, **kw), pad_ref)
    _same_dict(ops.pack_tokens_indexed_device(corpus, coffs, **sel, **kw, **caps), pack_ref)
    n = pad_ref["input_ids"].shape[0]
    need = ops.device_plan_bytes(n) + ops.device_batch_bytes(n, seq_len, None, pdt)
    full, out = _guarded(need)
    got = ops.pad_tokens_indexed_device(corpus, coffs, **sel, **kw, out=out)
    torch.cuda.synchronize()
    _same_dict(got, pad_ref)
    _check_guards(full, need)
    R, M = pack_ref["input_ids"].shape[0], pack_ref["cu_seqlens"].numel() - 1
    need = ops.device_plan_bytes(n, M, R) + ops.device_batch_bytes(R, seq_len, M, pdt)
    full, out = _guarded(need)
    got = ops.pack_tokens_indexed_device(corpus, coffs, **sel, **kw, out=out, max_rows=R, max_segs=M)
    torch.cuda.synchronize()
    _same_dict(got, pack_ref)
    for v in got.values():  # everything is carved from the caller's buffer
        assert out.data_ptr() <= v.data_ptr() < out.data_ptr() + need
    _check_guards(full, need)
    n_rows, n_seg, n_tokens, _ = pack_ref["counts"].tolist()
    if n_rows >= 0:  # the tail of the fixed-capacity cu_seqlens: zero-length sequences at the token count
        assert bool((pack_ref["cu_seqlens"][n_seg + 1:] == n_tokens).all())
    return pack_ref


@pytest.mark.parametrize("seq_len", [6, 256, 512, 516])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_device_planned_ops_match_their_cpu_reference_bitwise(np_dtype, seq_len):
    """seq_len 6: no multiple of 4 (the per-element store path), many segments; 512: exactly one chunk; 516: a
    second chunk with one live lane. Both position dtypes. The index has repeats and selects more tokens than
    the corpus holds, so the capacities are the caller's: first exactly the batch's segments (no tail)."""
    toks, offs, idx = _ragged_corpus(np_dtype)
    sel = dict(index=torch.from_numpy(idx))
    segs = int(np.sum(-(-(offs[idx + 1] - offs[idx]) // seq_len)))
    ref = _check_device_ops(toks, offs, sel, seq_len, caps=dict(max_rows=segs, max_segs=segs))
    n_rows, n_seg = ref["counts"][:2].tolist()
    assert 0 < n_rows <= segs and n_seg == segs
    caps = dict(max_rows=n_rows + 3, max_segs=n_seg + 2)  # more padding rows, a tail of two entries
    ref = _check_device_ops(toks, offs, sel, seq_len, pdt=torch.int32, caps=caps)
    assert ref["input_ids"].shape[0] == n_rows + 3 and bool((ref["segment_ids"][n_rows:] == -1).all())


@pytest.mark.parametrize("n_seq,seq_len,global_search", [(1100, 37, False), (1100, 6, True), (1200, 37, True)])
@pytest.mark.parametrize("np_dtype", [np.int16, np.int32])
def test_device_plans_around_the_lds_cap_of_the_segment_search(np_dtype, n_seq, seq_len, global_search):
    """Sequences of lengths i % 13 in the order of a Feistel permutation. 1100 of them at seq_len 37 are 1015
    segments: staged in LDS. At seq_len 6 and with 1200 sequences the plan has more than 1023 segments: the
    global-memory search. The device decides by the n_seg it reads from the plan's counts."""
    offs = _lens_corpus(n_seq, 13)
    info = np.iinfo(np_dtype)
    toks = np.random.default_rng(9).integers(info.min, info.max, size=int(offs[-1]), dtype=np_dtype, endpoint=True)
    ref = _check_device_ops(toks, offs, dict(perm=FeistelPermutation(n_seq, seed=2, epoch=1)), seq_len)
    n_rows, n_seg, n_tokens, max_seg = ref["counts"].tolist()
    assert n_rows >= 0 and n_tokens == int(offs[-1]) and max_seg == min(12, seq_len)
    assert (n_seg + 1 > _native.hip().TOKEN_SEG_LDS_CAP) == global_search


def test_degenerate_device_planned_batches():
    toks, offs, idx = _ragged_corpus(np.int32)
    empty = torch.from_numpy(np.array([idx[0], idx[13], idx[0]]))  # only empty sequences: only padding rows
    ref = _check_device_ops(toks, offs, dict(index=empty), 16)
    assert ref["counts"].tolist() == [0, 0, 0, 0] and not ref["cu_seqlens"].any()
    ref = _check_device_ops(toks, offs, dict(index=torch.zeros(0, dtype=torch.int64)), 16)  # n = 0
    assert ref["counts"].tolist() == [0, 0, 0, 0]
    # a row capacity that is too small is reported, not overrun: n_rows = -1, every row padding
    ref = _check_device_ops(toks, offs, dict(index=torch.from_numpy(idx)), 16, caps=dict(max_rows=3, max_segs=400))
    assert ref["counts"][0].item() == -1 and not ref["attention_mask"].any()


# ------------------------------------------------------------------- loader
def _corpus(token_dtype):
    return SharedTokenSource.synthetic(f"ddl_amd_rtpg_{np.random.randint(1 << 30)}", 200, 0, 300, seed=3,
                                       vocab=65536, token_dtype=token_dtype)


def _same(a: dict, b: dict) -> None:
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k].cpu(), b[k].cpu()), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


def _same_as_host_plan(dev: dict, host: dict, mode: str, max_segments: int) -> None:
    for k in ("input_ids", "attention_mask", "position_ids") + (("segment_ids",) if mode == "pack" else ()):
        assert dev[k].dtype == host[k].dtype and torch.equal(dev[k].cpu(), host[k].cpu()), k
    assert int(dev["n_tokens"]) == host["n_tokens"]
    if mode == "pack":
        n_seg = host["cu_seqlens"].numel() - 1
        assert int(dev["n_rows"]) == host["n_rows"] and int(dev["n_seg"]) == n_seg
        cu = dev["cu_seqlens"].cpu()
        assert cu.numel() == max_segments + 1 and torch.equal(cu[:n_seg + 1], host["cu_seqlens"].cpu())
        assert bool((cu[n_seg + 1:] == host["n_tokens"]).all())
        assert dev["max_seqlen"] >= host["max_seqlen"]


def _all(corpus, n_epochs, seq_len, mode, rank=0, world=1, clone=False, **kw):
    dl = ddl_amd.ResidentTokenLoader(corpus, GB, seq_len, mode, DDLEnv(rank=rank, world_size=world), seed=4,
                                     n_epochs=n_epochs, **kw)
    out = []
    for _ in range(n_epochs):
        for b in dl:
            out.append({k: v.clone() if clone and isinstance(v, torch.Tensor) else v for k, v in b.items()})
    torch.cuda.synchronize()
    return dl, out


@pytest.mark.parametrize("seq_len,mode,token_dtype,depth,rank,world", [
    (100, "pad", "uint16", 1, 0, 1),
    (256, "pack", "int32", 2, 1, 2),
    (100, "pack", "uint16", 1, 0, 1),
    (256, "pad", "int32", 2, 1, 2),
])
def test_device_plan_loader_equals_its_cpu_twin_and_the_host_plan(seq_len, mode, token_dtype, depth, rank, world):
    """Two epochs: the Feistel round keys change at the epoch boundary."""
    corpus = _corpus(token_dtype)
    try:
        _, twin = _all(corpus, 2, seq_len, mode, rank, world, device="cpu", plan="device")
        host_dl, host = _all(corpus, 2, seq_len, mode, rank, world, clone=True, plan="host", token_rows="fixed",
                             depth=depth)
        host_dl.close()
        dl, got = _all(corpus, 2, seq_len, mode, rank, world, clone=True, plan="device", depth=depth,
                       chunk_bytes=4096)
        assert len(got) == len(twin) == len(host) == 24
        for a, b, c in zip(got, twin, host):
            assert a["input_ids"].is_cuda and a["n_tokens"].is_cuda and a["n_tokens"].dim() == 0
            _same(a, b)
            _same_as_host_plan(a, c, mode, dl.layout.max_segments)
        st = dl.stats()
        assert st["plan"] == "device" and st["batches"] == 24 and st["handoff"] == "device"
        assert dl.timing()["host_us_per_step"] > 0
        dl.close()
        dl.close()  # harmless
    finally:
        corpus.close()


@pytest.mark.parametrize("mode", ["pad", "pack"])
def test_held_device_plan_batches_are_memory_of_their_own(mode):
    """depth = 1: two plan windows. Every batch of an epoch (12: each one is held across more than depth + 3
    further steps) is kept, not cloned, and compared at the end -- tensors, cu_seqlens and the count scalars."""
    corpus = _corpus("uint16")
    try:
        _, twin = _all(corpus, 1, 100, mode, device="cpu", plan="device")
        dl, held = _all(corpus, 1, 100, mode, plan="device", depth=1)
        assert len(held) == len(twin) == 12
        for a, b in zip(held, twin):
            _same(a, b)
        dl.close()
    finally:
        corpus.close()


@pytest.mark.parametrize("handoff", ["host", "device"])
def test_device_plan_handoff_modes_deliver_the_same_bytes_behind_a_busy_stream(handoff):
    corpus = _corpus("int32")
    try:
        _, twin = _all(corpus, 1, 256, "pack", device="cpu", plan="device")
        dl = ddl_amd.ResidentTokenLoader(corpus, GB, 256, "pack", seed=4, n_epochs=1, depth=3, handoff=handoff,
                                         plan="device")
        outs = []
        for g, b in enumerate(dl):
            if g % 4 == 0:
                torch.cuda._sleep(2_000_000)  # the consumer's stream is busy; later batches finish first
            outs.append({k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in b.items()})
        del b
        assert len(outs) == len(twin)
        for a, r in zip(outs, twin):
            _same(a, r)
        st = dl.stats()
        assert st["handoff"] == handoff and (st["host_waits"] == 0 or handoff == "host")
        dl.close()
    finally:
        corpus.close()
