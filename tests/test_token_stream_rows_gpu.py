"""The shuffled-row plan of the token stream on the GPU: ``stream_tokens_indexed_device(row_perm= / row_index=)``
(``token_stream_plan_rows`` + the emit kernel) against ``ops.ref_stream_tokens`` on the CPU, bit for bit, in
exact-size buffers between sentinel guards, and ``ResidentTokenStreamLoader(shuffle_rows=True)`` against its CPU
twin."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import _native, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation, row_seed_for
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A
KEYS = ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "counts")


def _guarded(need):
    full = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert full.data_ptr() % 16 == 0
    return full, full[GUARD:GUARD + need]


def _check_guards(full, need):
    host = full.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + need:] == SENTINEL).all())


def _stream_corpus(S, n, tail, dtype, seed):
    """Documents of lengths drawn from {0, 1, S - 1, S, S + 1, 3S + 2}, and a last one that makes T % S == tail."""
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, S - 1, S, S + 1, 3 * S + 2], size=n).astype(np.int64)
    lens[-1] = (tail - int(lens[:-1].sum())) % S + S
    return _from_lens(lens, dtype, rng)


def _from_lens(lens, dtype="int32", rng=None):
    rng = rng or np.random.default_rng(0)
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


class _Case:
    """A corpus on both sides, its table for one document order, and the runs of row selections over it."""

    def __init__(self, toks, offs, perm):
        self.toks, self.offs, self.perm = toks, offs, perm
        self.toks_d, self.offs_d = toks.cuda(), offs.cuda()
        self.table = ops.token_stream_table(self.offs_d, perm)
        self.T = int(offs[-1])

    def run(self, sel, rows, S, max_segs, pdt=torch.int64, labels=False):
        """``sel``: an int64 array (``row_index``) or ``(row_perm, row_base)``."""
        kw = dict(perm=self.perm, rows=rows, seq_len=S, pad_id=3, max_segs=max_segs, position_dtype=pdt,
                  labels=labels, ignore_index=-9)
        if isinstance(sel, tuple):
            ref_kw = dev_kw = dict(row_perm=sel[0], row_base=sel[1])
        else:
            idx = torch.from_numpy(np.asarray(sel, dtype=np.int64))
            ref_kw, dev_kw = dict(row_index=idx, row_base=0), dict(row_index=idx.cuda(), row_base=0)
        ref = ops.ref_stream_tokens(self.toks, self.offs, **ref_kw, **kw)
        need = sum(ops.token_stream_bytes(rows, S, max_segs, pdt, labels, shuffled_rows=True))
        full, out = _guarded(need)
        got = ops.stream_tokens_indexed_device(self.toks_d, self.offs_d, self.table, out=out,
                                               stream_rows=self.T // S, **dev_kw, **kw)
        torch.cuda.synchronize()
        _same(got, ref, KEYS + (("labels",) if labels else ()))
        _check_guards(full, need)
        return ref, got


def _special_rows(offs, perm, S):
    """A stream row lying wholly inside one document and not starting it, and one that starts on a document."""
    o = offs.numpy()
    n = o.size - 1
    q = np.arange(n) if perm is None else perm(np.arange(n))
    table = np.concatenate([[0], np.cumsum(o[q + 1] - o[q])])
    inside = boundary = None
    for r in range(1, int(table[-1]) // S):
        d = int(np.searchsorted(table, r * S, side="right")) - 1
        if table[d] < r * S and (r + 1) * S <= table[d + 1] and inside is None:
            inside = r
        if table[d] == r * S and boundary is None:
            boundary = r
    assert inside is not None and boundary is not None
    return inside, boundary


@pytest.mark.parametrize("dtype", ["int32", "uint16"])
@pytest.mark.parametrize("rows", [1, 3, 17])  # 17: one more row than a workgroup has waves
@pytest.mark.parametrize("S", [8, 6, 516])  # vector stores, the scalar path, two chunks per row
def test_row_plan_and_emit_equal_the_reference(S, rows, dtype):
    n = 64
    # a partial last row; the seeds are ones whose corpora hold both special rows in either document order
    toks, offs = _stream_corpus(S, n, 3, dtype, seed=S + rows + 5)
    lens = np.diff(offs.numpy())
    full_rows = int(offs[-1]) // S
    assert full_rows >= 2 * rows
    cap = ops.stream_max_segments(lens, rows, S, shuffled_rows=True)
    rng = np.random.default_rng(rows)
    case_no = 0
    for perm in (None, FeistelPermutation(n, seed=5, epoch=2)):
        case = _Case(toks, offs, perm)
        inside, boundary = _special_rows(offs, perm, S)
        special = np.concatenate([[inside, boundary], rng.permutation(full_rows)])
        special = special[np.sort(np.unique(special, return_index=True)[1])][:rows]  # distinct, the two in front
        row_perm = FeistelPermutation(full_rows, seed=7, epoch=1)
        selections = [
            (np.arange(rows), cap), (np.arange(full_rows - 1, full_rows - 1 - rows, -1), cap), (special, cap),
            (np.array(([inside, boundary, inside] * rows)[:rows]), rows * S),  # repeated rows: the caller's capacity
            ((row_perm, 0), cap), ((row_perm, full_rows - rows), cap),
        ]
        for sel, max_segs in selections:
            pdt = torch.int64 if case_no % 2 == 0 else torch.int32
            ref, got = case.run(sel, rows, S, max_segs, pdt, labels=case_no % 3 != 0)
            case_no += 1
            assert ref["counts"].tolist()[0] == rows and int(ref["counts"][1]) <= max_segs
        if rows == 1:
            assert int(case.run(np.array([inside]), 1, S, cap)[0]["counts"][1]) == 1  # first = last document
        # the identity selection is the contiguous path, tensor for tensor on the GPU
        ident = ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, perm=perm, row_base=0,
                                                 rows=rows, seq_len=S, max_segs=cap, labels=True,
                                                 row_index=torch.arange(rows).cuda())
        contiguous = ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, perm=perm, row_base=0,
                                                      rows=rows, seq_len=S, max_segs=cap, labels=True)
        assert list(ident) == list(contiguous)
        for k in ident:
            assert ident[k].is_cuda and torch.equal(ident[k], contiguous[k]), k
        # the op's own allocation and default capacity, stream_rows read from the table
        got = ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, perm=perm, row_base=1, rows=rows,
                                               seq_len=S, row_perm=row_perm)
        _same(got, ops.ref_stream_tokens(toks, offs, perm=perm, row_base=1, rows=rows, seq_len=S, row_perm=row_perm),
              KEYS)


def test_1025_rows_cross_a_tile_of_the_prefix_reduction():
    S, rows, n = 8, 1025, 3000
    toks, offs = _stream_corpus(S, n, 5, "uint16", seed=4)
    full_rows = int(offs[-1]) // S
    assert full_rows > rows
    cap = ops.stream_max_segments(np.diff(offs.numpy()), rows, S, shuffled_rows=True)
    case = _Case(toks, offs, FeistelPermutation(n, seed=3, epoch=0))
    ref, _ = case.run((FeistelPermutation(full_rows, seed=2, epoch=5), full_rows - rows), rows, S, cap, labels=True)
    assert ref["counts"].tolist()[0] == rows
    case.run(np.arange(full_rows - 1, full_rows - 1 - rows, -1), rows, S, cap, torch.int32)


def test_a_run_of_200_empty_documents_inside_one_row():
    S = 8
    lens = np.array([3] + [0] * 200 + [9] + [0] * 70 + [4, 8, 0, 0, 13, 2], dtype=np.int64)  # T = 39
    toks, offs = _from_lens(lens)
    case = _Case(toks, offs, None)
    cap = ops.stream_max_segments(lens, 4, S, shuffled_rows=True)
    ref, _ = case.run(np.array([0, 3, 1, 2]), 4, S, cap, labels=True)
    # row 0 = document 0 and, 201 documents on, the head of document 201; row 1 = its tail and document 272
    assert ref["cu_seqlens"][:2].tolist() == [0, 3] and ref["counts"].tolist()[0] == 4
    case.run(np.array([1]), 1, S, 3)


def test_more_than_1024_segments_and_hundreds_of_documents_per_row():
    rows, S, n = 3, 512, 2400
    rng = np.random.default_rng(2)
    lens = rng.integers(1, 3, size=n).astype(np.int64)
    toks, offs = _from_lens(lens, rng=rng)
    cap = ops.stream_max_segments(lens, rows, S, shuffled_rows=True)
    full_rows = int(offs[-1]) // S
    for perm in (None, FeistelPermutation(n, seed=1, epoch=0)):
        case = _Case(toks, offs, perm)
        for sel in (np.array([full_rows - 1, 1, 5]), (FeistelPermutation(full_rows, 9, 0), 0)):
            ref, _ = case.run(sel, rows, S, cap, labels=True)
            # more segments than the emit kernel stages in LDS
            assert int(ref["counts"][1]) > 1024 and int(ref["counts"][1]) + 1 > _native.hip().TOKEN_SEG_LDS_CAP


@pytest.mark.parametrize("S,rows", [(8, 3), (6, 1), (8, 17)])
def test_capacity_exceeded_by_one(S, rows):
    toks, offs = _stream_corpus(S, 300, 3, "int32", seed=7)
    case = _Case(toks, offs, FeistelPermutation(300, seed=2, epoch=1))
    full_rows = int(offs[-1]) // S
    row_perm = FeistelPermutation(full_rows, seed=4, epoch=0)
    segs = [int(ops.ref_stream_tokens(toks, offs, perm=case.perm, row_base=b, rows=rows, seq_len=S,
                                      row_perm=row_perm)["counts"][1]) for b in range(8)]
    base = int(np.argmax(segs))
    n_seg = segs[base]
    assert n_seg >= 2
    fit, _ = case.run((row_perm, base), rows, S, n_seg, labels=True)
    assert fit["counts"].tolist()[:2] == [rows, n_seg]
    over, _ = case.run((row_perm, base), rows, S, n_seg - 1, labels=True)
    assert over["counts"].tolist() == [-1, n_seg, rows * S, int(fit["counts"][3])]
    assert not over["attention_mask"].any() and not over["cu_seqlens"].any() and bool((over["labels"] == -9).all())


@pytest.mark.parametrize("rows,at", [(1, 0), (3, 1), (17, 16), (20, 0)])
def test_one_invalid_row_makes_the_batch_padding(rows, at):
    S = 8
    toks, offs = _stream_corpus(S, 120, 3, "int32", seed=11)
    case = _Case(toks, offs, FeistelPermutation(120, seed=1, epoch=1))
    full_rows = case.T // S
    good = np.random.default_rng(rows).permutation(full_rows)[:rows]
    valid = np.delete(good, at)
    want = [0, 0, 0, 0]
    if valid.size:
        c = ops.ref_stream_tokens(toks, offs, perm=case.perm, row_base=0, rows=valid.size, seq_len=S,
                                  max_segs=rows * S, row_index=valid)["counts"].tolist()
        want = [-1, c[1], valid.size * S, c[3]]
    else:
        want[0] = -1
    for bad in (-1, full_rows, 1 << 50):  # negative, the partial last row, far past the end
        sel = good.copy()
        sel[at] = bad
        ref, _ = case.run(sel, rows, S, rows * S, labels=True)
        assert ref["counts"].tolist() == want
        assert not ref["attention_mask"].any() and not ref["cu_seqlens"].any() and bool((ref["labels"] == -9).all())


def test_refused_arguments():
    toks, offs = _stream_corpus(8, 20, 0, "int32", seed=1)
    case = _Case(toks, offs, None)
    full_rows = case.T // 8
    kw = dict(row_base=0, rows=2, seq_len=8)
    idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="not both"):
        ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, row_index=idx,
                                         row_perm=FeistelPermutation(full_rows, 0, 0), **kw)
    with pytest.raises(TypeError, match="int64"):
        ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, row_index=idx.to(torch.int32), **kw)
    with pytest.raises(ValueError, match="device"):
        ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, row_index=idx.cpu(), **kw)
    with pytest.raises(ValueError, match="2 entries"):
        ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table,
                                         row_index=torch.zeros(3, dtype=torch.int64, device="cuda"), **kw)
    with pytest.raises(ValueError, match="row_base"):
        ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, row_index=idx, row_base=1, rows=2,
                                         seq_len=8)
    for stream_rows in (None, full_rows):  # read from the table, or given
        with pytest.raises(IndexError, match="full rows"):
            ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, stream_rows=stream_rows,
                                             row_perm=FeistelPermutation(full_rows - 1, 0, 0), **kw)
    with pytest.raises(IndexError, match="out of range"):
        ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, row_base=full_rows - 1, rows=2,
                                         seq_len=8, row_perm=FeistelPermutation(full_rows, 0, 0))
    with pytest.raises(ValueError, match="out must be"):
        need = sum(ops.token_stream_bytes(2, 8, 6))  # the contiguous plan's size: too small for the row plan
        assert need < sum(ops.token_stream_bytes(2, 8, 6, shuffled_rows=True))
        ops.stream_tokens_indexed_device(case.toks_d, case.offs_d, case.table, row_index=idx, max_segs=6,
                                         out=torch.empty(need, dtype=torch.uint8, device="cuda"), **kw)
    h = _native.hip()
    plan = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    args = dict(table=case.table.data_ptr(), corpus_offsets=case.offs_d.data_ptr(), n_corpus=20, n=20, mode=0, idx=0,
                base=0, keys=[0] * 6, n_domain=1, half_bits=1, stream_rows=full_rows, rows=2, seq_len=8, max_segs=8,
                seg_offsets=plan.data_ptr(), seg_src=plan.data_ptr() + 256, row_start=plan.data_ptr() + 512,
                row_end=plan.data_ptr() + 768, counts=plan.data_ptr() + 1024, scratch=plan.data_ptr() + 2048,
                stream=torch.cuda.current_stream().cuda_stream)
    rp = FeistelPermutation(full_rows, 0, 0).device_args()
    rows_ok = dict(rows_mode=2, rows_idx=0, rows_base=0, **{"rows_" + k: v for k, v in rp.items()})
    h.token_stream_plan_rows(**args, **rows_ok)  # accepted as it stands
    for change in (dict(rows=0), dict(scratch=0), dict(table=0), dict(rows=1 << 29), dict(stream_rows=full_rows + 1),
                   dict(rows=full_rows + 1)):
        with pytest.raises(ValueError, match="token_stream_plan_rows: unsupported arguments"):
            h.token_stream_plan_rows(**{**args, **change}, **rows_ok)
    with pytest.raises(ValueError, match="token_stream_plan_rows: unsupported arguments"):
        h.token_stream_plan_rows(**args, **dict(rows_ok, rows_base=full_rows - 1))
    torch.cuda.synchronize()


# ------------------------------------------------------------------- loader
def test_loader_with_shuffled_rows_equals_its_cpu_twin_over_two_epochs():
    GB, S = 8, 256
    src = SharedTokenSource.synthetic(f"ddl_amd_tsrg_{np.random.randint(1 << 30)}", 2000, 0, 600, seed=8,
                                      vocab=65536, token_dtype="uint16")
    try:
        kw = dict(seed=6, labels=True, shuffle_rows=True)
        dev = ddl_amd.ResidentTokenStreamLoader(src, GB, S, DDLEnv(), device="cuda", n_epochs=2, **kw)
        cpu = ddl_amd.ResidentTokenStreamLoader(src, GB, S, DDLEnv(), device="cpu", **kw)
        assert len(dev) == len(cpu) == dev.total_tokens // S // GB
        assert dev.max_segments == cpu.max_segments == ops.stream_max_segments(
            np.diff(src.offsets.tensor().view(-1).numpy()), GB, S, shuffled_rows=True)
        held = None
        first_rows = []
        for epoch in range(2):
            n = 0
            for a, b in zip(dev, cpu):
                assert list(a) == list(b) and "labels" in a
                for k in b:
                    if isinstance(b[k], torch.Tensor):
                        assert a[k].is_cuda and a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k]), (k, n)
                    else:
                        assert a[k] == b[k], k
                assert int(a["n_rows"]) == GB and int(a["n_tokens"]) == GB * S
                if n == 0:
                    first_rows.append(b["input_ids"].clone())
                if held is None:
                    held = (a, {k: v.clone() for k, v in a.items() if isinstance(v, torch.Tensor)})
                if epoch == 0 and n == dev.depth + 2:  # the held batch owns its memory: the rings have turned
                    for k, v in held[1].items():
                        assert torch.equal(held[0][k], v), k
                n += 1
            assert n == cpu.order.batches_per_epoch
        assert not torch.equal(first_rows[0], first_rows[1])
        assert dev.tables_built == 2  # still one table per epoch
        st = dev.stats()
        assert st["format"] == "stream" and st["shuffle_rows"] is True
        sd = dev.state_dict()
        assert sd["kind"] == "token_stream" and sd["epoch"] == 2 and sd["global_batch_cursor"] == 0
        assert sd["shuffle_rows"] is True and sd["row_seed"] == row_seed_for(6) == cpu.state_dict()["row_seed"]
        dev.close()
        cpu.close()
    finally:
        src.close()
