"""The weighted mix of corpus parts on the GPU: the ``token_mix_order`` kernel against ``ops.ref_mix_order`` bit for
bit in exact-size buffers between sentinel guards, the launcher's refusals, the table, plan and emit kernels run on
an order (``order=``) against the stream of the corpus materialised in that order, and
``ResidentTokenStreamLoader(mix=...)`` against its CPU twin across epoch boundaries."""

import os

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import TokenMix, _native, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A
KEYS = ("input_ids", "attention_mask", "position_ids", "segment_ids", "cu_seqlens", "counts", "labels")


def _guarded(need):
    full = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert full.data_ptr() % 16 == 0
    return full, full[GUARD:GUARD + need]


def _check_guards(full, need):
    host = full.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + need:] == SENTINEL).all())


def _from_lens(lens, dtype="int32", seed=0):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    toks = rng.integers(1, 60000, size=int(offs[-1]), dtype=np.int32)
    t = torch.from_numpy(toks)
    if dtype == "uint16":
        t = torch.from_numpy(toks.astype(np.uint16).view(np.int16))
    return t, torch.from_numpy(offs)


def materialise(toks, offs, order):
    """The epoch as a fresh corpus: tokens and offsets concatenated in ``order``."""
    o, t = offs.numpy(), toks.numpy()
    lens = o[order + 1] - o[order]
    new = np.concatenate([t[o[q]:o[q + 1]] for q in order] + [np.zeros(0, dtype=t.dtype)])
    return torch.from_numpy(new), torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


# ------------------------------------------------------------------ the order kernel
def _mixes(n_order):
    """Mixes of exactly ``n_order`` entries: one part once; (2.5, 1, 0.25); a one-document part three times; a part
    that does not appear between two others; 16 parts."""
    if n_order == 1:
        return [TokenMix([0, 1], [1.0]), TokenMix([0, 5, 6], [0.0, 1.0]), TokenMix([0, 2], [0.5])]
    b = n_order - 110
    mixes = [TokenMix([0, n_order], [1.0]),
             TokenMix([0, 40, 40 + b, 80 + b], [2.5, 1.0, 0.25]),
             TokenMix([0, 10, 11, n_order - 2], [1.0, 3.0, 1.0]),
             TokenMix([0, n_order - 60, n_order - 10, n_order + 30], [1.0, 0.0, 1.5]),
             TokenMix(list(range(0, 32, 2)) + [30 + n_order - 105], [0.5 * p for p in range(15)] + [1.0])]
    assert mixes[-1].parts == 16
    return mixes


@pytest.mark.parametrize("n_order", [1, 255, 256, 257, 513])  # one lane, and either side of one and two workgroups
def test_order_kernel_equals_the_reference_bit_for_bit(n_order):
    for mix in _mixes(n_order):
        assert mix.n_order == n_order
        for shuffle in (True, False):
            for epoch in (0, 1, 7):
                want = ops.ref_mix_order(mix, seed=13, epoch=epoch, shuffle=shuffle)
                full, inner = _guarded(8 * n_order)
                got = ops.token_mix_order(mix, seed=13, epoch=epoch, shuffle=shuffle, out=inner.view(torch.int64))
                torch.cuda.synchronize()
                assert got.is_cuda and got.dtype == torch.int64 and got.data_ptr() == inner.data_ptr()
                assert np.array_equal(got.cpu().numpy(), want), (mix, shuffle, epoch)
                _check_guards(full, 8 * n_order)
    # the op's own allocation
    got = ops.token_mix_order(mix, seed=2, epoch=3, device="cuda")
    assert np.array_equal(got.cpu().numpy(), ops.ref_mix_order(mix, seed=2, epoch=3))


def test_refused_arguments_launch_nothing():
    h = _native.hip()
    mix = TokenMix([0, 40, 60, 100], [2.5, 1.0, 0.25])
    full, inner = _guarded(8 * mix.n_order)
    parts = mix.device_args(5, True)
    outer = ops.row_selector(None, FeistelPermutation(mix.n_order, 5, 0), 0)
    args = dict(n_corpus=100, n=mix.n_order, order=inner.data_ptr(), stream=torch.cuda.current_stream().cuda_stream,
                **parts, **outer)
    h.token_mix_order(**args)  # accepted as it stands
    torch.cuda.synchronize()
    assert np.array_equal(inner.view(torch.int64).cpu().numpy(), ops.ref_mix_order(mix, seed=5, epoch=0))
    inner.fill_(SENTINEL)
    cbase = parts["cbase"]
    changes = [
        dict(cbase=[], doc_lo=[], n_docs=[], full_span=[], inner_keys=[], inner_half_bits=[]),  # no part
        dict(cbase=list(range(18)), doc_lo=list(range(17)), n_docs=[1] * 17, full_span=[1] * 17,
             inner_keys=[[0] * 6] * 17, inner_half_bits=[1] * 17, n=17),  # 17 parts
        dict(cbase=[1] + cbase[1:]),  # cbase[0] != 0
        dict(cbase=cbase[:1] + [cbase[1] - 30] + cbase[2:]),  # fewer entries than the whole passes
        dict(cbase=cbase[:1] + [cbase[1] + 30] + cbase[2:]),  # more extras than the part has documents
        dict(cbase=cbase[:3] + [cbase[3] + 1]),  # n is not cbase[parts]
        dict(n=mix.n_order - 1),
        dict(n_corpus=99),  # the last part ends outside the corpus
        dict(doc_lo=[-1, 40, 60]),
        dict(n_docs=[40, 0, 40]),
        dict(full_span=[81, 20, 0]),  # no whole number of passes
        dict(order=0),
        dict(base=1),  # positions [1, n + 1) leave the outer permutation's domain
        dict(n_domain=mix.n_order - 1),
        dict(half_bits=0),
        dict(mode=3),
        dict(mode=1, idx=0),
        dict(inner_half_bits=[0, 3, 3]),  # part 0 has extras: its keys must permute its 40 documents
        dict(inner_half_bits=[2, 3, 3]),  # 2^(2 * 2) < 40
        dict(inner_half_bits=[3, 3, 33]),
        dict(inner_keys=parts["inner_keys"][:2], inner_half_bits=parts["inner_half_bits"][:2]),
    ]
    for change in changes:
        with pytest.raises(ValueError, match="token_mix_order|index mode 1"):
            h.token_mix_order(**{**args, **change})
    torch.cuda.synchronize()
    assert bool((inner.cpu() == SENTINEL).all())  # nothing was launched
    # a part without extras needs no valid inner keys; without the inner shuffle none are read
    h.token_mix_order(**{**args, "inner_half_bits": [3, 0, 3]})
    torch.cuda.synchronize()
    assert np.array_equal(inner.view(torch.int64).cpu().numpy(), ops.ref_mix_order(mix, seed=5, epoch=0))
    h.token_mix_order(**{**args, "inner_shuffle": False, "inner_keys": [], "inner_half_bits": []})
    torch.cuda.synchronize()
    assert inner.view(torch.int64).cpu().tolist() == _inner_identity(mix, 5)
    _check_guards(full, 8 * mix.n_order)


def _inner_identity(mix, seed):
    """The order with the epoch's outer permutation and identity inner ones, by the written-out sequence."""
    seq = ops.ref_mix_order(mix, seed=seed, epoch=0, shuffle=False)
    return seq[FeistelPermutation(mix.n_order, seed, 0)(np.arange(mix.n_order))].tolist()


# ------------------------------------------------------------------ table, plan and emit on an order
def _same(got, ref):
    assert tuple(got) == KEYS
    for k in KEYS:
        g = got[k].cpu()
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, k
        assert torch.equal(g, ref[k]), k


class _Case:
    """A corpus on both sides, a mix's epoch order written by the kernel, its table, and the corpus materialised in
    that order: the reference of every run is ``ref_stream_tokens`` of the materialised corpus with no order at all."""

    def __init__(self, lens, mix, dtype, shuffle, seed=3, epoch=1):
        self.toks, self.offs = _from_lens(lens, dtype, seed)
        self.toks_d, self.offs_d = self.toks.cuda(), self.offs.cuda()
        self.order_d = ops.token_mix_order(mix, seed=seed, epoch=epoch, shuffle=shuffle, device="cuda")
        self.order = self.order_d.cpu().numpy()
        assert np.array_equal(self.order, ops.ref_mix_order(mix, seed=seed, epoch=epoch, shuffle=shuffle))
        self.mt, self.mo = materialise(self.toks, self.offs, self.order)
        self.T = int(self.mo[-1])
        assert self.T == mix.epoch_tokens(lens, seed, shuffle)
        n = self.order.size
        full, inner = _guarded(8 * (n + 1))
        self.table = ops.token_stream_table(self.offs_d, order=self.order_d, out=inner.view(torch.int64))
        torch.cuda.synchronize()
        assert torch.equal(self.table.cpu(), self.mo)
        _check_guards(full, 8 * (n + 1))

    def run(self, rows, S, max_segs, row_base=0, row_perm=None, pdt=torch.int64):
        kw = dict(row_base=row_base, rows=rows, seq_len=S, pad_id=3, max_segs=max_segs, position_dtype=pdt,
                  labels=True, ignore_index=-9, row_perm=row_perm)
        ref = ops.ref_stream_tokens(self.mt, self.mo, perm=None, **kw)
        need = sum(ops.token_stream_bytes(rows, S, max_segs, pdt, True, shuffled_rows=row_perm is not None))
        full, out = _guarded(need)
        got = ops.stream_tokens_indexed_device(self.toks_d, self.offs_d, self.table, order=self.order_d, out=out,
                                               stream_rows=self.T // S, **kw)
        torch.cuda.synchronize()
        _same(got, ref)
        _check_guards(full, need)
        return ref


@pytest.mark.parametrize("dtype", ["int32", "uint16"])
@pytest.mark.parametrize("S", [8, 16])
def test_table_plan_and_emit_on_an_order_equal_the_materialised_corpus(S, dtype):
    rng = np.random.default_rng(S)
    lens = rng.choice([0, 1, S - 1, S, S + 1, 3 * S + 2], size=90).astype(np.int64)
    lens[40] = 1  # a one-token document, five times over
    mix = TokenMix([0, 40, 41, 60, 90], [2.5, 5.0, 0.0, 0.25])
    rows = 5
    for shuffle in (False, True):
        case = _Case(lens, mix, dtype, shuffle)
        full_rows = case.T // S
        assert full_rows > 3 * rows
        cap = ops.stream_max_segments(np.repeat(lens, mix.document_copies()), rows, S)
        cap_rows = ops.stream_max_segments(np.repeat(lens, mix.document_copies()), rows, S, shuffled_rows=True)
        for k, base in enumerate((0, 7, full_rows - 2, full_rows + 3)):  # the last two: a window past the end
            ref = case.run(rows, S, cap, row_base=base, pdt=torch.int32 if k % 2 else torch.int64)
            assert int(ref["counts"][0]) == max(0, min(rows, -(-(case.T - base * S) // S)))
        row_perm = FeistelPermutation(full_rows, seed=9, epoch=2)
        for base in (0, full_rows - rows):
            assert case.run(rows, S, cap_rows, row_base=base, row_perm=row_perm)["counts"].tolist()[0] == rows
        if not shuffle:
            # the five copies of the one-token document lie side by side: five segments of one token, each at position 0
            at = int(np.flatnonzero(case.order == 40)[0])
            assert case.order[at:at + 5].tolist() == [40] * 5
            t0 = int(case.mo[at])
            r0 = t0 // S
            ref = case.run(2, S, 2 * S, row_base=r0)
            local = t0 - r0 * S
            flat_pos, flat_seg = ref["position_ids"].view(-1), ref["segment_ids"].view(-1)
            assert flat_pos[local:local + 5].tolist() == [0] * 5
            assert len(set(flat_seg[local:local + 5].tolist())) == 5
            assert len(set(ref["input_ids"].view(-1)[local:local + 5].tolist())) == 1
            ref = case.run(1, S, S, row_base=0, row_perm=FeistelPermutation(full_rows, 1, 0))
        # one segment more than the capacity: n_rows = -1 and a batch of padding
        n_seg = int(case.run(rows, S, cap, row_base=2)["counts"][1])
        over = case.run(rows, S, n_seg - 1, row_base=2)
        assert over["counts"].tolist()[:3] == [-1, n_seg, rows * S] and not over["attention_mask"].any()
        assert not over["cu_seqlens"].any() and bool((over["labels"] == -9).all())
        n_seg = int(case.run(rows, S, cap_rows, row_perm=row_perm)["counts"][1])
        over = case.run(rows, S, n_seg - 1, row_perm=row_perm)
        assert over["counts"].tolist()[:3] == [-1, n_seg, rows * S] and not over["attention_mask"].any()


def test_refused_order_arguments():
    toks, offs = _from_lens(np.full(10, 9))
    toks_d, offs_d = toks.cuda(), offs.cuda()
    order = torch.arange(10, device="cuda")
    table = ops.token_stream_table(offs_d, order=order)
    kw = dict(row_base=0, rows=2, seq_len=8)
    with pytest.raises(ValueError, match="not both"):
        ops.stream_tokens_indexed_device(toks_d, offs_d, table, order=order, perm=FeistelPermutation(10, 0, 0), **kw)
    with pytest.raises(ValueError, match="not both"):
        ops.token_stream_table(offs_d, FeistelPermutation(10, 0, 0), order=order)
    with pytest.raises(TypeError, match="int64"):
        ops.stream_tokens_indexed_device(toks_d, offs_d, table, order=order.to(torch.int32), **kw)
    with pytest.raises(ValueError, match="device"):
        ops.stream_tokens_indexed_device(toks_d, offs_d, table, order=order.cpu(), **kw)
    with pytest.raises(ValueError, match="table must be"):  # an order longer than the table
        ops.stream_tokens_indexed_device(toks_d, offs_d, table, order=torch.arange(11, device="cuda") % 10, **kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the loader
@pytest.mark.parametrize("shuffle_rows", [False, True])
def test_loader_with_a_mix_equals_its_cpu_twin_across_epoch_boundaries(shuffle_rows):
    GB, S = 8, 64
    rng = np.random.default_rng(6)
    lens = rng.choice([0, 1, S - 1, S, S + 1, 3 * S + 2], size=24).astype(np.int64)
    mix = TokenMix([0, 8, 9, 16, 24], [1.5, 3.0, 0.0, 0.25])
    toks, offs = _from_lens(lens, "uint16", seed=6)
    src = SharedTokenSource.create(f"ddl_amd_tmixg_{os.getpid()}_{int(shuffle_rows)}", toks.numpy().view(np.uint16),
                                   offs.numpy(), "uint16")
    try:
        kw = dict(seed=6, labels=True, shuffle_rows=shuffle_rows, mix=mix, depth=2)
        dev = ddl_amd.ResidentTokenStreamLoader(src, GB, S, DDLEnv(), device="cuda", n_epochs=3, **kw)
        cpu = ddl_amd.ResidentTokenStreamLoader(src, GB, S, DDLEnv(), device="cpu", n_epochs=3, **kw)
        # fewer batches per epoch than the prefetch depth + 1: prefetch crosses the boundary, both order slots live
        assert 1 <= len(dev) == len(cpu) == dev.total_tokens // S // GB < dev.depth + 1
        assert dev.total_tokens == cpu.total_tokens == mix.epoch_tokens(lens, 6)
        assert dev.max_segments == cpu.max_segments
        firsts = []
        for epoch in range(3):
            n = 0
            for a, b in zip(dev, cpu):
                assert list(a) == list(b) and "labels" in a
                for k in b:
                    if isinstance(b[k], torch.Tensor):
                        assert a[k].is_cuda and a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k]), (epoch, n, k)
                    else:
                        assert a[k] == b[k], k
                assert int(a["n_rows"]) == GB and int(a["n_tokens"]) == GB * S
                if n == 0:
                    firsts.append(b["input_ids"].clone())
                n += 1
            assert n == cpu.batches_per_epoch
            if epoch == 0:  # the next epoch's order was built while this one's was still being read
                assert dev.stats()["orders_built"] >= 2
        assert not torch.equal(firsts[0], firsts[1])
        st = dev.stats()
        assert st["orders_built"] == st["tables_built"] == 3  # one per epoch touched
        assert st["mix_parts"] == 4 and st["mix_documents"] == mix.n_order
        sd = dev.state_dict()
        assert sd["mix"] == cpu.state_dict()["mix"] == mix.state() and sd["epoch"] == 3
        dev.close()
        cpu.close()
    finally:
        src.close()
