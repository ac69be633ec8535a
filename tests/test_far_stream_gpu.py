"""The token plan kernels on values past 2^32 and 2^40 without any token memory (csrc/kernels/tokens_plan.hip,
tokens_stream.hip, tokens_stream_rows.hip, tokens_mix.hip): a corpus of 8 documents of 2^40 tokens among short and
empty ones, so that the stream table, the plans' ``seg_src`` and the descriptor's ``src_start`` reach 2^43 (plan
outputs compared, nothing emitted), and a ``TokenMix`` whose ``n_corpus``, ``cbase`` and order length pass 2^32.
References: plain loops over the offsets here, and the definition of ``ops.ref_mix_order`` evaluated entry by entry
with the scalar Feistel reference (checked against ``ops.ref_mix_order`` itself on a small mix)."""

import numpy as np
import pytest
import torch

from ddl_amd import _native, ops
from ddl_amd.permutation import FeistelPermutation, part_seed_for
from ddl_amd.token_mix import TokenMix
from tests import far_refs as FR
from tests import feistel_ref

pytestmark = pytest.mark.gpu

BIG_DOC = 1 << 40
LENS = np.array([5, BIG_DOC, 0, 7, BIG_DOC, BIG_DOC, 1, (1 << 32) + 3, BIG_DOC, 0, 0, BIG_DOC, 4097, BIG_DOC, BIG_DOC,
                 3, BIG_DOC, 11], dtype=np.int64)
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
N = len(LENS)
PERM = FeistelPermutation(N, seed=21, epoch=1)
SENT = -(0x5A5A5A5A5A5A5A5A)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _st():
    return torch.cuda.current_stream().cuda_stream


def _order():
    return np.array([feistel_ref.py_perm(i, N, 21, 1) for i in range(N)], dtype=np.int64)


def _table():
    return np.concatenate([[0], np.cumsum(LENS[_order()])]).astype(np.int64)


def test_stream_table_to_2_43():
    offs = torch.from_numpy(OFFS).to(_dev())
    table = _table()
    assert table[-1] > 1 << 43
    buf = torch.full((N + 3,), SENT, dtype=torch.int64, device=_dev())
    got = ops.token_stream_table(offs, PERM, out=buf[1:N + 2])
    assert got.cpu().numpy().tolist() == table.tolist()
    assert buf[0].item() == SENT and buf[N + 2].item() == SENT
    assert ops.token_stream_table(offs).cpu().numpy().tolist() == OFFS.tolist()  # identity order


def _pieces(rows_g, S):
    """Segments of the stream rows that start at stream positions ``rows_g``: (batch-local start, corpus element,
    length) per maximal run of one document inside one row, and the token count. Positions at or past T hold none."""
    order, table = _order(), _table()
    T = int(table[-1])
    segs, n_tok = [], 0
    for k, g0 in enumerate(rows_g):
        g = g0
        while g < min(g0 + S, T):
            d = int(np.searchsorted(table, g, side="right")) - 1
            end = min(int(table[d + 1]), g0 + S, T)
            segs.append((k * S + (g - g0), int(OFFS[order[d]]) + (g - int(table[d])), end - g))
            n_tok += end - g
            g = end
    return segs, n_tok


def _plan_buffers(rows, M):
    d = _dev()
    return {k: torch.full((n,), SENT, dtype=torch.int64, device=d)
            for k, n in (("seg_offsets", M + 2), ("seg_src", M + 1), ("row_start", rows + 1), ("row_end", rows + 1),
                         ("counts", 5), ("scratch", 4 * rows + 1))}


def _check_plan(b, segs, n_tok, rows, S, M, row_limits, what):
    got = {k: v.cpu().numpy() for k, v in b.items()}
    n_seg = len(segs)
    assert n_seg <= M
    assert got["seg_offsets"][:n_seg].tolist() == [s[0] for s in segs], what
    assert got["seg_offsets"][n_seg] == n_tok and (got["seg_offsets"][n_seg + 1:] == SENT).all(), what
    assert got["seg_src"][:n_seg].tolist() == [s[1] for s in segs], what
    assert (got["seg_src"][n_seg:] == SENT).all(), what
    assert got["row_start"][:rows].tolist() == [a for a, _ in row_limits], what
    assert got["row_end"][:rows].tolist() == [e for _, e in row_limits], what
    assert got["row_start"][rows] == SENT and got["row_end"][rows] == SENT and got["counts"][4] == SENT, what
    assert got["counts"][:4].tolist() == [-(-n_tok // S), n_seg, n_tok, max([s[2] for s in segs], default=0)], what


@pytest.mark.parametrize("S", [6, 512])
def test_stream_plans_on_2_40_token_documents(S):
    """``token_stream_plan`` at row bases whose ``row_base * S`` passes 2^32, 2^40 and 2^43 and across every document
    border, and ``token_stream_plan_rows`` selecting the rows on both sides of those places."""
    h, d = _native.hip(), _dev()
    offs = torch.from_numpy(OFFS).to(d)
    table_np = _table()
    table = torch.from_numpy(table_np).to(d)
    T = int(table_np[-1])
    sel = ops.row_selector(None, PERM, 0)
    common = dict(table=table.data_ptr(), corpus_offsets=offs.data_ptr(), n_corpus=N, n=N, seq_len=S, stream=_st())
    bases = [-(-(1 << 32) // S), (1 << 40) // S, (1 << 43) // S - 1, T // S - 1] + [max(int(t) // S - 1, 0) for t in table_np[1:-1]]
    rows, M = 3, 3 * 8
    for row_base in bases:
        b = _plan_buffers(rows, M)
        h.token_stream_plan(row_base=row_base, rows=rows, max_segs=M, seg_offsets=b["seg_offsets"].data_ptr(),
                            seg_src=b["seg_src"].data_ptr(), row_start=b["row_start"].data_ptr(),
                            row_end=b["row_end"].data_ptr(), counts=b["counts"].data_ptr(), **common, **sel)
        torch.cuda.synchronize()
        segs, n_tok = _pieces([(row_base + r) * S for r in range(rows)], S)
        limits = [(min(r * S, n_tok), min((r + 1) * S, n_tok)) for r in range(rows)]
        _check_plan(b, segs, n_tok, rows, S, M, limits, f"plan S={S} row_base={row_base}")
    rho = sorted({min(max(x + k, 0), T // S - 1) for x in bases for k in (-1, 0, 1, 2)} | {0})
    rho = list(np.random.default_rng(2).permutation(rho))
    rows, M = len(rho), len(rho) * 8
    index = torch.tensor(rho, dtype=torch.int64, device=d)
    b = _plan_buffers(rows, M)
    h.token_stream_plan_rows(stream_rows=T // S, rows=rows, max_segs=M, seg_offsets=b["seg_offsets"].data_ptr(),
                             seg_src=b["seg_src"].data_ptr(), row_start=b["row_start"].data_ptr(),
                             row_end=b["row_end"].data_ptr(), counts=b["counts"].data_ptr(),
                             scratch=b["scratch"].data_ptr(), **common, **sel,
                             **{"rows_" + k: v for k, v in ops.row_selector(index, None, 0).items()})
    torch.cuda.synchronize()
    segs, n_tok = _pieces([int(r) * S for r in rho], S)
    assert n_tok == rows * S
    _check_plan(b, segs, n_tok, rows, S, M, [(r * S, (r + 1) * S) for r in range(rows)], f"row plan S={S}")
    assert b["scratch"][4 * rows].item() == SENT


@pytest.mark.parametrize("S", [1 << 30, (1 << 39) + 1])
def test_batch_descriptor_on_2_40_token_documents(S):
    """``token_batch_descriptor``: ``src_start`` and ``seg_src`` to 2^43, the batch's running offsets past 2^41."""
    h, d = _native.hip(), _dev()
    offs = torch.from_numpy(OFFS).to(d)
    idx = np.array([16, 3, 1, 9, 7, 0, 13, 2, 4, 17, 16, 8], dtype=np.int64)
    n = len(idx)
    starts, lens = OFFS[idx], LENS[idx]
    seg_src = [int(s) + j * S for s, ln in zip(starts, lens) for j in range(-(-int(ln) // S))]
    M = len(seg_src) + 3
    out = {k: torch.full((m,), SENT, dtype=torch.int64, device=d)
           for k, m in (("src_start", n + 1), ("offsets", n + 2), ("seg_src", M), ("counts", 5))}
    index = torch.from_numpy(idx).to(d)
    h.token_batch_descriptor(corpus_offsets=offs.data_ptr(), n_corpus=N, n=n, seq_len=S, max_segs=M,
                             src_start=out["src_start"].data_ptr(), offsets=out["offsets"].data_ptr(),
                             seg_src=out["seg_src"].data_ptr(), counts=out["counts"].data_ptr(), pad_counts=False,
                             stream=_st(), **ops.row_selector(index, None, 0))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got["src_start"].tolist() == starts.tolist() + [SENT]
    assert got["offsets"].tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist() + [SENT]
    assert got["offsets"][n] > 1 << 41
    assert got["seg_src"].tolist() == seg_src + [SENT] * 3 and max(seg_src) > 1 << 43
    assert got["counts"][2:].tolist() == [int(lens.sum()), int(min(lens.max(), S)), SENT]


# ------------------------------------------------------------------- mix order
def _mix_entry(mix, i, seed, epoch):
    """``ops.ref_mix_order``'s definition for one entry, in Python integers with the scalar Feistel reference."""
    v = feistel_ref.py_perm(i, mix.n_order, seed, epoch)
    p = max(q for q in range(mix.parts) if mix.cbase[q] <= v)
    while mix.cbase[p + 1] <= v:  # parts without entries share their cbase with the next one
        p += 1
    j = v - mix.cbase[p]
    span = mix.full[p] * mix.n_docs[p]
    if j < span:
        return mix.bounds[p] + j % mix.n_docs[p]
    return mix.bounds[p] + feistel_ref.py_perm(j - span, mix.n_docs[p], part_seed_for(seed, p), 0)


def test_mix_entry_definition_equals_ref_mix_order():
    mix = TokenMix([0, 100, 157, 300], [2.5, 0.0, 1.25])
    ref = ops.ref_mix_order(mix, seed=5, epoch=3)
    assert [_mix_entry(mix, i, 5, 3) for i in range(mix.n_order)] == ref.tolist()


def test_mix_order_past_2_32():
    """A mix over 2^32 + 500 documents whose order holds more than 2^32 entries (``cbase`` past 2^32, an inner
    permutation of 2^32 - 500 documents): the kernel writes the whole order (about 43 GB), sampled entries at the
    marks, the part borders and hash-chosen places equal the definition."""
    mix = TokenMix([0, 1000, (1 << 32) + 500], [3.5, 1.25])
    n = mix.n_order
    assert mix.cbase[-1] > 1 << 32 and mix.n_documents > 1 << 32 and mix.extra[1] > 1 << 29
    FR.need_hbm(8 * n)
    out = torch.empty(n + 2, dtype=torch.int64, device=_dev())
    out[0], out[n + 1] = SENT, SENT
    got = ops.token_mix_order(mix, seed=7, epoch=2, out=out[1:n + 1])
    torch.cuda.synchronize()
    at = {0, 1, n - 1, n - 2} | {m + k for m in (1 << 31, 1 << 32) for k in (-1, 0, 1)}
    at |= {int(x) for x in np.random.default_rng(4).integers(0, n, 400)}
    span1 = mix.cbase[1] + mix.full[1] * mix.n_docs[1]  # where part 1's whole pass ends and its extras begin
    for v in (0, 999, 1000, mix.cbase[1] - 1, mix.cbase[1], mix.cbase[1] + 1, span1 - 1, span1, span1 + 1, n - 1):
        at.add(feistel_ref.py_position(v, n, 7, 2))  # the entries that hold the part and pass borders
    at = sorted(at)
    vals = got[torch.tensor(at, dtype=torch.int64, device=_dev())].cpu().tolist()
    ref = [_mix_entry(mix, i, 7, 2) for i in at]
    assert vals == ref
    assert max(ref) > 1 << 32 and sum(r < 1000 for r in ref) >= 4
    assert out[0].item() == SENT and out[n + 1].item() == SENT
    lo, hi = 0, 0
    for c in range(0, n, FR.FILL_CHUNK):  # every entry inside the corpus
        part = got[c:c + FR.FILL_CHUNK]
        lo, hi = min(lo, int(part.min())), max(hi, int(part.max()))
    assert lo >= 0 and hi < mix.n_documents
    del out, got
    torch.cuda.empty_cache()
