"""Next-token labels of the token paths on the CPU: the reference against a plain double loop, every op's CPU path
and the ``device="cpu"`` loaders against the reference, the output carving, and the host check of the kernel's
label arithmetic (csrc/kernels/tests/token_labels_check.cpp under ASan/UBSan)."""

import os
import shutil

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.types import DDLEnv
from tests.host_check import run_host_check

S = 37
GB = 12


def loop_labels(ids, mask, seg, ignore):
    """The definition, position by position."""
    shape = tuple(ids.shape)
    ids, mask = ids.tolist(), mask.tolist()
    seg = seg.tolist() if seg is not None else None
    out = [[ignore] * len(row) for row in ids]
    for r, row in enumerate(ids):
        for p in range(len(row) - 1):
            if mask[r][p + 1] == 1 and (seg is None or seg[r][p + 1] == seg[r][p]):
                out[r][p] = row[p + 1]
    return torch.tensor(out, dtype=torch.int64).reshape(shape)


def check_labels(batch_or_tuple, pack, ignore=-100):
    """``labels`` of a batch equals the reference of the batch's own other outputs (and the plain loop)."""
    if isinstance(batch_or_tuple, dict):
        b = batch_or_tuple
        ids, mask, seg, lab = b["input_ids"], b["attention_mask"], b.get("segment_ids"), b["labels"]
    else:
        ids, mask, seg, lab = batch_or_tuple[0], batch_or_tuple[1], batch_or_tuple[3] if pack else None, \
            batch_or_tuple[-1]
    assert (seg is not None) == pack
    assert lab.dtype == torch.int64 and lab.shape == ids.shape
    assert torch.equal(lab, ops.ref_token_labels(ids, mask, seg, ignore))
    assert torch.equal(lab, loop_labels(ids, mask, seg, ignore))


# ------------------------------------------------------------------ 1. the reference
def test_ref_token_labels_against_a_plain_loop_on_hand_built_batches():
    # pack mode, S = 8: a segment ending at the last column, a one-token segment, an empty sequence between two
    # others (it leaves no segment: ids 0 -> 1 are neighbours), a padding row
    ids = torch.tensor([[11, 12, 13, 21, 31, 32, 33, 34],
                        [41, 42, 51, 52, 53, 0, 0, 0],
                        [0, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    mask = torch.tensor([[1] * 8, [1] * 5 + [0] * 3, [0] * 8], dtype=torch.uint8)
    seg = torch.tensor([[0, 0, 0, 1, 2, 2, 2, 2], [3, 3, 4, 4, 4, -1, -1, -1], [-1] * 8], dtype=torch.int32)
    for ignore in (-100, -7, 0):
        lab = ops.ref_token_labels(ids, mask, seg, ignore)
        i = ignore
        assert lab.tolist() == [[12, 13, i, i, 32, 33, 34, i], [42, i, 52, 53, i, i, i, i], [i] * 8]
        assert lab.dtype == torch.int64 and torch.equal(lab, loop_labels(ids, mask, seg, ignore))
    # pad mode: a row longer than S (truncated: its last position has no target), a short row, an empty row
    ids = torch.tensor([[1, 2, 3, 4], [5, 6, 9, 9], [9, 9, 9, 9]], dtype=torch.int32)
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]], dtype=torch.uint8)
    assert ops.ref_token_labels(ids, mask).tolist() == [[2, 3, 4, -100], [6, -100, -100, -100], [-100] * 4]
    assert torch.equal(ops.ref_token_labels(ids, mask, None, 5), loop_labels(ids, mask, None, 5))
    # no rows, one column
    assert ops.ref_token_labels(ids[:0], mask[:0]).shape == (0, 4)
    assert ops.ref_token_labels(ids[:, :1], mask[:, :1]).tolist() == [[-100]] * 3
    # the pad-mode batch of real ops: a sequence longer than S, one of S, empty ones
    toks = torch.arange(100, 100 + 3 * S, dtype=torch.int32)
    offs = torch.tensor([0, S + 5, S + 5, 2 * S + 5, 2 * S + 6, 3 * S], dtype=torch.int64)
    out = ops.pad_tokens(toks, offs, S, pad_id=3, labels=True, ignore_index=-7)
    check_labels(out, False, -7)
    assert out[3][0, S - 1] == -7 and out[3][0, S - 2] == toks[S - 1] and (out[3][1] == -7).all()
    assert (out[3][3] == -7).all()  # a one-token sequence has no target


# ------------------------------------------------------------------ 2. the ops' CPU paths
@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 3 * S + 1, size=60)
    lens[[0, 1, 2, 3, 4, 5, 6]] = [0, 1, S - 1, S, S + 1, 2 * S + 3, 0]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = rng.integers(0, 60000, size=int(offs[-1]), dtype=np.int32)
    return torch.from_numpy(toks), torch.from_numpy(offs)


def _bitwise(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.parametrize("tok_dtype", [torch.int32, torch.int16])
@pytest.mark.parametrize("seq_len", [16, S])
def test_every_op_on_cpu_tensors(ragged, seq_len, tok_dtype):
    toks, offs = ragged
    toks = toks.to(tok_dtype)
    n = offs.numel() - 1
    for idx in (np.arange(n), np.array([5, 0, 59, 5, 17, 42, 6]), np.array([0, 6]), np.array([], dtype=np.int64)):
        flat, dofs = ops.ref_gather_ragged(toks, offs, idx)
        for ignore in (-100, -7):
            kw = dict(labels=True, ignore_index=ignore)
            # flat ops
            off = ops.pad_tokens(flat, dofs, seq_len, 9)
            on = ops.pad_tokens(flat, dofs, seq_len, 9, **kw)
            assert len(on) == 4
            _bitwise(on[:3], off)
            check_labels(on, False, ignore)
            off = ops.pack_tokens(flat, dofs, seq_len, 9)
            on = ops.pack_tokens(flat, dofs, seq_len, 9, **kw)
            assert len(on) == 6
            _bitwise(on[:5], off)
            check_labels(on, True, ignore)
            # indexed ops
            off = ops.pad_tokens_indexed(toks, offs, idx, seq_len, 9)
            on = ops.pad_tokens_indexed(toks, offs, idx, seq_len, 9, **kw)
            assert len(on) == 4
            _bitwise(on[:3], off)
            check_labels(on, False, ignore)
            for fill in (0, 70):
                off = ops.pack_tokens_indexed(toks, offs, idx, seq_len, 9, fill_rows=fill)
                on = ops.pack_tokens_indexed(toks, offs, idx, seq_len, 9, fill_rows=fill, **kw)
                assert len(on) == 6
                _bitwise(on[:5], off)
                check_labels(on, True, ignore)
                if fill:
                    assert on[0].shape[0] == max(fill, off[0].shape[0])
            # device-planned ops (an index, and the identity), and an overflowing plan
            index = torch.from_numpy(idx.astype(np.int64))
            for sel in (dict(index=index), dict(base=0, count=min(len(idx), n))):
                off = ops.pad_tokens_indexed_device(toks, offs, seq_len=seq_len, pad_id=9, **sel)
                on = ops.pad_tokens_indexed_device(toks, offs, seq_len=seq_len, pad_id=9, **sel, **kw)
                assert set(on) == set(off) | {"labels"}
                for k in off:
                    assert torch.equal(on[k], off[k]), k
                check_labels(on, False, ignore)
                off = ops.pack_tokens_indexed_device(toks, offs, seq_len=seq_len, pad_id=9, **sel)
                on = ops.pack_tokens_indexed_device(toks, offs, seq_len=seq_len, pad_id=9, **sel, **kw)
                assert set(on) == set(off) | {"labels"}
                for k in off:
                    assert torch.equal(on[k], off[k]), k
                check_labels(on, True, ignore)
            if len(idx) > 6:
                on = ops.pack_tokens_indexed_device(toks, offs, index=index, seq_len=seq_len, max_rows=2, **kw)
                assert int(on["counts"][0]) == -1 and (on["labels"] == ignore).all() and on["labels"].shape[0] == 2
            on = ops.pack_tokens_device(flat, dofs, seq_len, 9, **kw)
            off = ops.pack_tokens_device(flat, dofs, seq_len, 9)
            assert set(on) == set(off) | {"labels"}
            check_labels(on, True, ignore)
    with pytest.raises(ValueError):
        ops.pad_tokens(toks, offs, seq_len, labels=True, ignore_index=1 << 31)
    assert len(ops.pad_tokens(toks, offs, seq_len, ignore_index=1 << 40)) == 3  # unused without labels


# token_output_bytes(labels=False) of the parent commit, for (rows, S, n_seg, position dtype)
PARENT_BYTES = {
    (3, 37, 5, torch.int64): 1936, (3, 37, None, torch.int32): 1008, (0, 16, 0, torch.int64): 16,
    (2, 512, 1, torch.int32): 13328, (64, 4096, 90, torch.int64): 4456816, (1, 1, None, torch.int64): 48,
    (7, 515, 1100, torch.int64): 65744, (5, 16, None, torch.int64): 1040,
}


def test_carving_with_labels_keeps_the_other_views_and_appends_an_aligned_region():
    for (rows, s, n_seg, pdt), parent in PARENT_BYTES.items():
        assert ops.token_output_bytes(rows, s, n_seg, pdt) == parent
        assert ops.token_output_bytes(rows, s, n_seg, pdt, labels=False) == parent
        need = ops.token_output_bytes(rows, s, n_seg, pdt, labels=True)
        assert need == parent + -(-8 * rows * s // 16) * 16
        assert ops.device_batch_bytes(rows, s, n_seg, pdt) == parent + 32
        assert ops.device_batch_bytes(rows, s, n_seg, pdt, labels=True) == need + 32
        whole = torch.zeros(need, dtype=torch.uint8)
        off = ops.carve_token_outputs(whole, rows, s, n_seg, pdt)
        on = ops.carve_token_outputs(whole, rows, s, n_seg, pdt, labels=True)
        assert len(off) == 5 and len(on) == 6
        for a, b in zip(off, on):  # the existing views, at their offsets
            assert (a is None) == (b is None)
            if a is not None:
                assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype
        lab = on[5]
        assert lab.dtype == torch.int64 and lab.shape == (rows, s)
        if lab.numel():
            lo = lab.data_ptr() - whole.data_ptr()
            assert lo % 16 == 0 and lo + 8 * rows * s <= need
            for t in on[:5]:  # overlaps nothing: behind every other region
                if t is not None and t.numel():
                    assert t.data_ptr() - whole.data_ptr() + t.numel() * t.element_size() <= lo
            assert lo == parent  # right behind the mask, the last region without labels


# ------------------------------------------------------------------ 3. the loaders' CPU twins
@pytest.fixture(scope="module", params=["int32", "uint16"])
def corpus(request, ragged):
    toks, offs = ragged
    src = SharedTokenSource.create(f"ddl_amd_tl_{os.getpid()}_{request.param}", toks.numpy(), offs.numpy(),
                                   request.param)
    yield src
    src.close()


def _loader(cls, corpus, mode, **kw):
    return cls(corpus, GB, S, mode, DDLEnv(rank=0, world_size=1), device="cpu", seed=4, **kw)


def _same(a: dict, b: dict, keys=None) -> None:
    if keys is None:
        assert a.keys() == b.keys()
    for k in (keys or a):
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("token_rows", ["exact", "fixed"])
@pytest.mark.parametrize("mode,pack_order", [("pad", "in_order"), ("pack", "in_order"), ("pack", "ffd")])
def test_cpu_loaders_deliver_labels_only_when_asked(corpus, mode, pack_order, token_rows):
    kw = dict(pack_order=pack_order, token_rows=token_rows)
    pack = mode == "pack"
    rt = _loader(ddl_amd.ResidentTokenLoader, corpus, mode, labels=True, ignore_index=-7, **kw)
    zc = _loader(ddl_amd.ZeroCopyTokenLoader, corpus, mode, labels=True, ignore_index=-7, **kw)
    plain = _loader(ddl_amd.ResidentTokenLoader, corpus, mode, **kw)
    plain_zc = _loader(ddl_amd.ZeroCopyTokenLoader, corpus, mode, **kw)
    dev = dev_plain = None
    if pack_order == "in_order" and (not pack or token_rows == "fixed"):
        dev = _loader(ddl_amd.ResidentTokenLoader, corpus, mode, plan="device", labels=True, ignore_index=-7, **kw)
        dev_plain = _loader(ddl_amd.ResidentTokenLoader, corpus, mode, plan="device", **kw)
    assert rt.stats().keys() == plain.stats().keys() and zc.stats().keys() == plain_zc.stats().keys()
    assert len(rt) == 5
    tensors = ["input_ids", "attention_mask", "position_ids"] + (["segment_ids"] if pack else [])
    for _ in range(2):  # two epochs
        got, ref, off, off_zc = list(rt), list(zc), list(plain), list(plain_zc)
        assert len(got) == len(ref) == len(off) == len(off_zc) == 5
        for a, b, c, d in zip(got, ref, off, off_zc):
            _same(a, b)  # the paths agree key by key
            assert "labels" not in c and "labels" not in d and set(a) == set(c) | {"labels"}
            _same(c, a, keys=c.keys())  # labels on changes nothing else
            check_labels(a, pack, -7)
        if dev is not None:
            on, no = list(dev), list(dev_plain)
            for a, b, c in zip(on, no, got):
                assert set(a) == set(b) | {"labels"}
                _same(b, a, keys=tensors)
                _same(a, c, keys=tensors + ["labels"])  # the device plan's twin agrees with the host plan's
                check_labels(a, pack, -7)
    for ld in (rt, zc, plain, plain_zc, dev, dev_plain):
        if ld is not None:
            ld.close()


def test_checkpoint_is_independent_of_labels(corpus):
    full = list(_loader(ddl_amd.ResidentTokenLoader, corpus, "pack", labels=True, n_epochs=1))
    on = _loader(ddl_amd.ResidentTokenLoader, corpus, "pack", labels=True, n_epochs=1)
    off = _loader(ddl_amd.ResidentTokenLoader, corpus, "pack", n_epochs=1)
    it_on, it_off = iter(on), iter(off)
    for _ in range(2):
        next(it_on), next(it_off)
    sd = on.state_dict()
    assert sd == off.state_dict()  # the same state dict, labels or not
    rest = list(_loader(ddl_amd.ZeroCopyTokenLoader, corpus, "pack", n_epochs=1, resume_state=sd))  # on -> off
    assert len(rest) == 3 and all("labels" not in b for b in rest)
    for a, b in zip(rest, full[2:]):
        _same(a, b, keys=a.keys())
    back = _loader(ddl_amd.ResidentTokenLoader, corpus, "pack", n_epochs=1, resume_state=off.state_dict(),
                   labels=True)  # and off -> on
    for a, b in zip(list(back), full[2:]):
        _same(a, b)
    with pytest.raises(ValueError):
        _loader(ddl_amd.ResidentTokenLoader, corpus, "pack", labels=True, ignore_index=-(1 << 31) - 1)


# ------------------------------------------------------------------ 4. the kernel's label arithmetic on the host
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_label_arithmetic_under_asan_ubsan(tmp_path):
    """ti_labels4 (csrc/kernels/tokens_indexed.h) replayed for every lane over exact-size heap buffers: a plain
    executable, nothing preloaded."""
    run_host_check(tmp_path, "token_labels_check", "token labels check ok")
