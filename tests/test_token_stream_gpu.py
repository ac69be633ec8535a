"""The token stream kernels on the GPU: ``token_stream_table`` against the NumPy cumulative sum,
``stream_tokens_indexed_device`` (plan + emit) against ``ops.ref_stream_tokens`` on the CPU, bit for bit, and
``ResidentTokenStreamLoader`` against its CPU twin."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import _native, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A
SENTINEL64 = int.from_bytes(bytes([SENTINEL]) * 8, "little")
KEYS = ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "counts")


def _guarded(need):
    full = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert full.data_ptr() % 16 == 0
    return full, full[GUARD:GUARD + need]


def _check_guards(full, need):
    host = full.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + need:] == SENTINEL).all())


# -------------------------------------------------------------------- table
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3 * 1024 + 7, 1024 * 1024 + 5])
def test_table_equals_the_numpy_cumulative_sum(n):
    lens = (np.arange(n, dtype=np.int64) * 7) % 5  # a fifth of the documents are empty
    lens[::11] += 4096
    coffs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    coffs_dev = torch.from_numpy(coffs).cuda()
    scratch_n = _native.hip().token_stream_table_scratch(n)
    assert scratch_n == max(1, -(-n // 1024))
    for perm in (None, FeistelPermutation(n, seed=9, epoch=3)):
        q = np.arange(n) if perm is None else perm(np.arange(n))
        want = np.concatenate([[0], np.cumsum(lens[q])]).astype(np.int64)
        # exact-size outputs between sentinels: table [n + 1] and the tile sums
        t_full, t_buf = _guarded(8 * (n + 1))
        s_full, s_buf = _guarded(8 * scratch_n)
        got = ops.token_stream_table(coffs_dev, perm, out=t_buf.view(torch.int64), scratch=s_buf.view(torch.int64))
        torch.cuda.synchronize()
        assert got.data_ptr() == t_buf.data_ptr() and got.shape == (n + 1,)
        assert np.array_equal(got.cpu().numpy(), want)
        _check_guards(t_full, 8 * (n + 1))
        _check_guards(s_full, 8 * scratch_n)
        assert np.array_equal(ops.token_stream_table(coffs_dev, perm).cpu().numpy(), want)  # its own allocations
        assert np.array_equal(ops.token_stream_table(torch.from_numpy(coffs), perm).numpy(), want)  # the CPU path


# ------------------------------------------------------------ plan and emit
def _stream_corpus(S, n, tail, dtype, seed):
    """Documents of lengths drawn from {0, 1, S - 1, S, S + 1, 3S + 2}, and a last one that makes T % S == tail."""
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, S - 1, S, S + 1, 3 * S + 2], size=n).astype(np.int64)
    lens[-1] = (tail - int(lens[:-1].sum())) % S + S
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = rng.integers(1, 60000, size=int(offs[-1]), dtype=np.int32)
    t = torch.from_numpy(toks)
    if dtype == "uint16":
        t = torch.from_numpy(toks.astype(np.uint16).view(np.int16))
    return t, torch.from_numpy(offs)


def _same(got, ref, keys):
    assert list(got) == list(keys)
    for k in keys:
        g = got[k].cpu()
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, k
        assert torch.equal(g, ref[k]), k


def _run_window(toks, offs, toks_d, offs_d, table, perm, row_base, rows, S, max_segs, pdt, labels):
    kw = dict(perm=perm, row_base=row_base, rows=rows, seq_len=S, pad_id=3, max_segs=max_segs, position_dtype=pdt,
              labels=labels, ignore_index=-9)
    ref = ops.ref_stream_tokens(toks, offs, **kw)
    need = sum(ops.token_stream_bytes(rows, S, max_segs, pdt, labels))
    full, out = _guarded(need)
    got = ops.stream_tokens_indexed_device(toks_d, offs_d, table, out=out, **kw)
    torch.cuda.synchronize()
    _same(got, ref, KEYS + (("labels",) if labels else ()))
    _check_guards(full, need)
    return ref


@pytest.mark.parametrize("dtype", ["int32", "uint16"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("S", [8, 6, 516])  # vector stores, the scalar path, two chunks per row
def test_plan_and_emit_equal_the_reference(S, rows, dtype):
    n = 48
    for tail in (0, 3):  # T a multiple of S (a window ends exactly at T), and a partial last row
        toks, offs = _stream_corpus(S, n, tail, dtype, seed=S + rows)
        T = int(offs[-1])
        assert T % S == tail
        toks_d, offs_d = toks.cuda(), offs.cuda()
        for perm in (None, FeistelPermutation(n, seed=5, epoch=2)):
            table = ops.token_stream_table(offs_d, perm)
            lens = np.diff(offs.numpy())
            cap = ops.stream_max_segments(lens, rows, S)
            last = T // S - rows  # tail == 0: ends exactly at T
            case = 0
            for row_base in (0, 1, last // 2, last, last + 1, T // S + 2):  # the last two reach past T
                for pdt in (torch.int64, torch.int32):
                    ref = _run_window(toks, offs, toks_d, offs_d, table, perm, row_base, rows, S, cap, pdt,
                                      labels=case % 2 == 0)
                    case += 1
                    assert int(ref["counts"][0]) >= 0 and int(ref["counts"][1]) <= cap
            # the op's own allocation and default capacity
            got = ops.stream_tokens_indexed_device(toks_d, offs_d, table, perm=perm, row_base=2, rows=rows, seq_len=S)
            _same(got, ops.ref_stream_tokens(toks, offs, perm=perm, row_base=2, rows=rows, seq_len=S), KEYS)


def test_more_than_1024_documents_and_segments_in_one_batch():
    rows, S, n = 3, 512, 2400
    rng = np.random.default_rng(2)
    lens = rng.integers(1, 3, size=n).astype(np.int64)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    toks = torch.from_numpy(rng.integers(1, 60000, size=int(offs[-1]), dtype=np.int32))
    toks_d, offs_d = toks.cuda(), offs.cuda()
    cap = ops.stream_max_segments(lens, rows, S)
    for perm in (None, FeistelPermutation(n, seed=1, epoch=0)):
        table = ops.token_stream_table(offs_d, perm)
        for row_base in (0, 1):
            ref = _run_window(toks, offs, toks_d, offs_d, table, perm, row_base, rows, S, cap, torch.int64, True)
            # two plan tiles, and more segments than the emit kernel stages in LDS
            assert int(ref["counts"][1]) > 1024 and int(ref["counts"][1]) + 1 > _native.hip().TOKEN_SEG_LDS_CAP


@pytest.mark.parametrize("S,rows", [(8, 3), (6, 1), (512, 3)])
def test_capacity_exceeded_by_one(S, rows):
    toks, offs = _stream_corpus(S, 300, 3, "int32", seed=7)
    if S == 512:  # more than a tile of documents
        lens = np.random.default_rng(3).integers(1, 3, size=2400).astype(np.int64)
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        toks = torch.arange(1, int(offs[-1]) + 1, dtype=torch.int32)
    toks_d, offs_d = toks.cuda(), offs.cuda()
    perm = FeistelPermutation(offs.numel() - 1, seed=2, epoch=1)
    table = ops.token_stream_table(offs_d, perm)
    segs = [int(ops.ref_stream_tokens(toks, offs, perm=perm, row_base=b, rows=rows, seq_len=S)["counts"][1])
            for b in range(1, 9)]
    base = 1 + int(np.argmax(segs))  # a window with at least two segments: a capacity of one less is still >= 1
    n_seg = segs[base - 1]
    assert n_seg >= 2
    fit = _run_window(toks, offs, toks_d, offs_d, table, perm, base, rows, S, n_seg, torch.int64, True)
    assert int(fit["counts"][0]) == rows
    over = _run_window(toks, offs, toks_d, offs_d, table, perm, base, rows, S, n_seg - 1, torch.int64, True)
    assert over["counts"].tolist() == [-1, n_seg, int(fit["counts"][2]), int(fit["counts"][3])]
    assert not over["attention_mask"].any() and not over["cu_seqlens"].any() and bool((over["labels"] == -9).all())


def test_refused_arguments():
    toks, offs = _stream_corpus(8, 20, 0, "int32", seed=1)
    toks_d, offs_d = toks.cuda(), offs.cuda()
    table = ops.token_stream_table(offs_d)
    with pytest.raises(ValueError, match="table"):
        ops.stream_tokens_indexed_device(toks_d, offs_d, None, row_base=0, rows=1, seq_len=8)
    with pytest.raises(ValueError, match="table"):
        ops.stream_tokens_indexed_device(toks_d, offs_d, table[:5], row_base=0, rows=1, seq_len=8)
    with pytest.raises(ValueError, match="int32 cu_seqlens"):
        ops.stream_tokens_indexed_device(toks_d, offs_d, table, row_base=0, rows=1 << 20, seq_len=1 << 12)
    with pytest.raises(IndexError):
        ops.stream_tokens_indexed_device(toks_d, offs_d, table, perm=FeistelPermutation(19, 0, 0), row_base=0, rows=1,
                                         seq_len=8)
    with pytest.raises(ValueError, match="out must be"):
        ops.stream_tokens_indexed_device(toks_d, offs_d, table, row_base=0, rows=1, seq_len=8,
                                         out=torch.empty(64, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------- loader
def test_loader_equals_its_cpu_twin_over_two_epochs():
    GB, S = 8, 256
    src = SharedTokenSource.synthetic(f"ddl_amd_tsg_{np.random.randint(1 << 30)}", 2000, 0, 600, seed=8,
                                      vocab=65536, token_dtype="uint16")
    try:
        other = ddl_amd.ResidentTokenLoader(src, GB, S, "pack", DDLEnv(), device="cuda", seed=6)
        dev = ddl_amd.ResidentTokenStreamLoader(src, GB, S, DDLEnv(), device="cuda", seed=6, labels=True, n_epochs=2)
        cpu = ddl_amd.ResidentTokenStreamLoader(src, GB, S, DDLEnv(), device="cpu", seed=6, labels=True)
        assert dev.replica_shared and dev.replica_ptr == other.replica_ptr  # one replica for both loaders
        assert len(dev) == len(cpu) == dev.total_tokens // S // GB
        held = None
        for epoch in range(2):
            n = 0
            for a, b in zip(dev, cpu):
                assert list(a) == list(b)
                for k in b:
                    if isinstance(b[k], torch.Tensor):
                        assert a[k].is_cuda and a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k]), (k, n)
                    else:
                        assert a[k] == b[k], k
                if held is None:
                    held = (a, {k: v.clone() for k, v in a.items() if isinstance(v, torch.Tensor)})
                if epoch == 0 and n == dev.depth + 2:  # the held batch owns its memory: the rings have turned
                    for k, v in held[1].items():
                        assert torch.equal(held[0][k], v), k
                n += 1
            assert n == cpu.order.batches_per_epoch
        assert dev.tables_built == 2  # one table per epoch, built when its first step is assembled
        assert dev.stats()["format"] == "stream"
        sd = dev.state_dict()
        assert sd["kind"] == "token_stream" and sd["epoch"] == 2 and sd["global_batch_cursor"] == 0
        dev.close()
        assert other.replica_ptr is not None  # the replica outlives the stream loader
        other.close()
        cpu.close()
    finally:
        src.close()
