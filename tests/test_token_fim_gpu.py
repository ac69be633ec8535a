"""Fill-in-the-middle rearrangement on the GPU: the ``token_fim`` kernel against ``ops.ref_fim_tokens`` bit for bit,
ids and labels, in exact-size buffers between sentinel guards (the grid of the CPU test, 64 rows of 1024, both
position widths, a capacity beyond the segments, segments across chunk and lane borders, corrupt batches), the
launcher's refusals, and both stream loaders with ``fim=`` against the CPU twin and each other."""

import os

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import TokenFIM, TokenMix, _native, ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.types import DDLEnv
from tests.test_token_fim import (EOD, GRID_SEED, MID, PRE, SUF, _corpus, grid_batches, grid_lens, my_keys,
                                  stream_elements)

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A


def _guarded(need):
    full = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert full.data_ptr() % 16 == 0
    return full, full[GUARD:GUARD + need]


def _check_guards(full, need):
    host = full.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + need:] == SENTINEL).all())


def _on_device(batch):
    return {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in batch.items()}


def _launch(dev, fim, keys_d, seed, epoch, labels=True, ignore_index=-100):
    """``token_fim`` into exact-size guarded buffers, through the launcher the ops and the loaders use."""
    R, S = dev["input_ids"].shape
    full_o, out = _guarded(4 * R * S)
    full_l, lab = _guarded(8 * R * S)
    from ddl_amd.ops.kernels import launch_fim

    launch_fim(_native.hip(), ids_ptr=dev["input_ids"].data_ptr(), seg=dev["segment_ids"], pos=dev["position_ids"],
               cu_ptr=dev["cu_seqlens"].data_ptr(), cap=min(dev["cu_seqlens"].numel() - 1, keys_d.numel()),
               seg_keys_ptr=keys_d.data_ptr(), counts_ptr=dev["counts"].data_ptr() if "counts" in dev else 0,
               out_ptr=out.data_ptr(), labels_ptr=lab.data_ptr() if labels else 0, ignore_index=ignore_index, rows=R,
               seq_len=S, fim_args=fim.device_args(seed, epoch), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check_guards(full_o, 4 * R * S)
    _check_guards(full_l, 8 * R * S)
    if not labels:
        assert bool((lab.cpu() == SENTINEL).all())
    return out.view(torch.int32).view(R, S).cpu(), lab.view(torch.int64).view(R, S).cpu()


def _check(batch, fim, keys, seed=1, epoch=2, what=None):
    keys = torch.as_tensor(np.asarray(keys, dtype=np.int64))
    ref = ops.ref_fim_tokens(batch, fim, seg_keys=keys, seed=seed, epoch=epoch, labels=True, ignore_index=-9)
    dev = _on_device(batch)
    out, lab = _launch(dev, fim, keys.cuda(), seed, epoch, ignore_index=-9)
    assert torch.equal(out, ref["input_ids"]), what
    assert torch.equal(lab, ref["labels"]), what
    return ref


# ------------------------------------------------------------------ the op against the reference
@pytest.mark.parametrize("eod", [None, EOD])
@pytest.mark.parametrize("S", [8, 10, 516])
def test_kernel_equals_the_reference_over_the_grid(S, eod):
    batches = grid_batches(S, eod)
    for min_len in (4, 8):
        seed = GRID_SEED[(S, eod is not None, min_len)]
        for rate in (0, 0.5, 1):
            for spm_rate in (0, 0.5, 1):
                fim = TokenFIM(rate, prefix_id=PRE, middle_id=MID, suffix_id=SUF, spm_rate=spm_rate, eod_id=eod,
                               min_len=min_len)
                for n, (b, keys) in enumerate(batches):
                    ref = _check(b, fim, keys, seed, 3, (S, eod, min_len, rate, spm_rate, n))
                    if rate == 1:
                        assert not torch.equal(ref["input_ids"], b["input_ids"])
    # the op: its own allocations, labels or none, every other entry the input's
    b, keys = batches[0]
    dev = _on_device(b)
    ref = ops.ref_fim_tokens(b, fim, seg_keys=np.asarray(keys), seed=seed, epoch=0, labels=True)
    got = ops.fim_tokens(dev, fim, seg_keys=torch.tensor(keys, device="cuda"), seed=seed, epoch=0, labels=True)
    assert got["input_ids"].is_cuda and torch.equal(got["input_ids"].cpu(), ref["input_ids"])
    assert got["labels"].dtype == torch.int64 and torch.equal(got["labels"].cpu(), ref["labels"])
    assert all(got[k] is dev[k] for k in dev if k != "input_ids")
    assert torch.equal(dev["input_ids"].cpu(), b["input_ids"])  # the input is not written
    got = ops.fim_tokens(dev, fim, seg_keys=torch.tensor(keys, device="cuda"), seed=seed, epoch=0)
    assert "labels" not in got and torch.equal(got["input_ids"].cpu(), ref["input_ids"])


@pytest.mark.parametrize("pdt", [torch.int32, torch.int64])
def test_64_rows_of_1024_with_a_capacity_beyond_the_segments(pdt):
    S, R = 1024, 64
    rng = np.random.default_rng(3)
    # segments across the 512-position chunk border (500 + 30, 1000 + 50) and across lanes' four positions (odd
    # lengths), short ones, and documents longer than a row
    lens = np.concatenate([[500, 30, 494, 1000, 50, 998, 7, 5, 4, 3, 1, 2 * S + 3],
                           rng.choice([1, 3, 4, 5, 9, 13, 511, 513, S - 1, S, S + 1, 3 * S + 2], size=160)])
    toks, offs = _corpus(lens, seed=3, eod=EOD, mid_doc=3)
    cap = ops.stream_max_segments(lens, R, S) + 100
    b = ops.ref_stream_tokens(toks, offs, row_base=0, rows=R, seq_len=S, max_segs=cap, position_dtype=pdt)
    n_seg = int(b["counts"][1])
    assert int(b["counts"][0]) == R and n_seg + 100 <= cap == b["cu_seqlens"].numel() - 1
    sid, pos = b["segment_ids"], b["position_ids"]
    assert bool(((sid[:, 511] == sid[:, 512]) & (pos[:, 512] > 0)).any())  # a segment straddles the chunk border
    assert bool((pos[:, 1::4] == 0).any() and (pos[:, 2::4] == 0).any() and (pos[:, 3::4] == 0).any())
    keys = my_keys(b, stream_elements(offs.numpy(), range(len(lens))), list(range(R)), S)
    keys = np.concatenate([np.asarray(keys, dtype=np.int64), np.full(cap - n_seg, -1, dtype=np.int64)])
    for spm_rate in (0.0, 1.0, 0.5):
        fim = TokenFIM(0.75, prefix_id=PRE, middle_id=MID, suffix_id=SUF, spm_rate=spm_rate, eod_id=EOD)
        ref = _check(b, fim, keys, what=(pdt, spm_rate))
        assert not torch.equal(ref["input_ids"], b["input_ids"])
    # int64 segment ids read the same
    b64 = dict(b, segment_ids=b["segment_ids"].to(torch.int64))
    assert torch.equal(_check(b64, fim, keys)["input_ids"], ref["input_ids"])


def test_an_overflowed_batch_and_corrupt_batches_touch_nothing_outside():
    toks, offs = _corpus(grid_lens(8), seed=1)
    fim = TokenFIM(1.0, prefix_id=PRE, middle_id=MID, suffix_id=SUF, min_len=4)
    over = ops.ref_stream_tokens(toks, offs, row_base=0, rows=5, seq_len=8, max_segs=2, labels=True)
    ref = _check(over, fim, np.zeros(2, dtype=np.int64))
    assert torch.equal(ref["input_ids"], over["input_ids"])
    b = ops.ref_stream_tokens(toks, offs, row_base=0, rows=5, seq_len=8)
    keys = np.arange(int(b["counts"][1]), dtype=np.int64)
    dead = dict(b, counts=torch.tensor([-1, 0, 0, 0]))
    assert torch.equal(_check(dead, fim, keys)["input_ids"], b["input_ids"])
    _check(b, fim, keys[:3])  # fewer keys than segments: the capacity is the keys'
    rng = np.random.default_rng(0)
    for c in range(20):  # whatever the arrays hold, the kernel equals the reference and leaves the guards alone
        w = {k: v.clone() for k, v in b.items()}
        at = rng.integers(0, 40, size=6)
        w["segment_ids"].view(-1)[at[:2]] = torch.tensor(rng.integers(-5, 60, size=2), dtype=torch.int32)
        w["position_ids"].view(-1)[at[2:4]] = torch.tensor(rng.integers(-9, 30, size=2))
        w["cu_seqlens"][rng.integers(0, w["cu_seqlens"].numel(), size=2)] = torch.tensor(
            rng.integers(-8, 90, size=2), dtype=torch.int32)
        if c % 4 == 0:
            w["position_ids"].view(-1)[at[4]] = (1 << 63) - 1
            w["position_ids"].view(-1)[at[5]] = -(1 << 63)
        ref = ops.ref_fim_tokens(w, fim, seg_keys=keys, seed=1, epoch=c)
        out, _ = _launch(_on_device(w), fim, torch.from_numpy(keys).cuda(), 1, c, labels=False)
        assert torch.equal(out, ref["input_ids"]), c


def test_refused_arguments_launch_nothing():
    b, keys = grid_batches(8, None)[0]
    dev = _on_device(b)
    keys_d = torch.tensor(keys, device="cuda")
    fim = TokenFIM(1.0, prefix_id=PRE, middle_id=MID, suffix_id=SUF)
    full, out = _guarded(4 * 40)
    h = _native.hip()
    args = dict(ids=dev["input_ids"].data_ptr(), seg=dev["segment_ids"].data_ptr(), seg_is_i64=False,
                pos=dev["position_ids"].data_ptr(), pos_is_i64=True, cu=dev["cu_seqlens"].data_ptr(),
                cap=keys_d.numel(), seg_keys=keys_d.data_ptr(), counts=0, out=out.data_ptr(), labels=0,
                ignore_index=-100, rows=5, seq_len=8, stream=torch.cuda.current_stream().cuda_stream,
                **fim.device_args(0, 0))
    h.token_fim(**args)  # accepted as it stands
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32).view(5, 8).cpu(),
                       ops.ref_fim_tokens(b, fim, seg_keys=np.asarray(keys), seed=0, epoch=0)["input_ids"])
    out.fill_(SENTINEL)
    for change in (dict(rows=0), dict(seq_len=0), dict(rows=1 << 20, seq_len=1 << 12), dict(ids=0), dict(out=0),
                   dict(seg=0), dict(pos=0), dict(cu=0), dict(seg_keys=0), dict(cap=-1), dict(min_len=3),
                   dict(rate_q=(1 << 24) + 1), dict(spm_q=(1 << 24) + 1), dict(out=out.data_ptr() + 4),
                   dict(out=dev["input_ids"].data_ptr()), dict(labels=dev["position_ids"].data_ptr()),
                   dict(ignore_index=1 << 31)):
        with pytest.raises(ValueError, match="token_fim"):
            h.token_fim(**{**args, **change})
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENTINEL).all())  # nothing was launched
    _check_guards(full, 4 * 40)
    with pytest.raises(TypeError, match="seg_keys"):
        ops.fim_tokens(dev, fim, seg_keys=keys, seed=0, epoch=0)
    with pytest.raises(ValueError, match="GPU"):
        ops.fim_tokens(dev, fim, seg_keys=torch.tensor(keys), seed=0, epoch=0)


# ------------------------------------------------------------------ the loaders
FIM = TokenFIM(0.5, prefix_id=PRE, middle_id=MID, suffix_id=SUF, eod_id=EOD, min_len=8)
CASES = [(S, shuffle_rows, labels, False) for S in (516, 1024) for shuffle_rows in (False, True)
         for labels in (False, True)] + [(516, True, True, True)]


def _same_batches(a, b, what):
    assert list(a) == list(b), what
    for k in b:
        if isinstance(b[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), (what, k)
        else:
            assert a[k] == b[k], (what, k)


@pytest.mark.parametrize("S,shuffle_rows,labels,mixed", CASES)
def test_both_loaders_equal_the_cpu_twin_over_two_epochs(S, shuffle_rows, labels, mixed):
    GB, n_docs = 8, 60
    rng = np.random.default_rng(S)
    lens = rng.choice([0, 1, 3, 4, 5, 100, S - 1, S, S + 1, 3 * S + 2], size=n_docs).astype(np.int64)
    toks, offs = _corpus(lens, seed=S, eod=EOD, mid_doc=int(np.argmax(lens)))
    mix = TokenMix([0, 20, 21, 40, n_docs], [1.5, 3.0, 0.0, 0.5]) if mixed else None
    src = SharedTokenSource.create(f"ddl_amd_tfimg_{os.getpid()}_{S}_{int(shuffle_rows)}{int(labels)}{int(mixed)}",
                                   toks.numpy().astype(np.uint16), offs.numpy(), "uint16")
    loaders = []
    try:
        kw = dict(seed=5, labels=labels, shuffle_rows=shuffle_rows, mix=mix, n_epochs=2)

        def make(cls, device, **more):
            loaders.append(cls(src, GB, S, DDLEnv(), device=device, **kw, **more))
            return loaders[-1]

        cpu = make(ddl_amd.ResidentTokenStreamLoader, "cpu", fim=FIM)
        res = make(ddl_amd.ResidentTokenStreamLoader, "cuda", fim=FIM)
        zc = make(ddl_amd.ZeroCopyTokenStreamLoader, "cuda", fim=FIM)
        plain_cpu = make(ddl_amd.ResidentTokenStreamLoader, "cpu")
        plain = make(ddl_amd.ResidentTokenStreamLoader, "cuda")  # without fim, in the same process
        assert res.stats()["fim"] and zc.stats()["fim"] and not plain.stats()["fim"]
        assert len(cpu) == len(res) == len(zc) == len(plain) >= 2
        moved = 0
        for epoch in range(2):
            n = 0
            for c, r, z, pc, p in zip(cpu, res, zc, plain_cpu, plain):
                _same_batches(r, c, ("resident", epoch, n))
                _same_batches(z, c, ("zero-copy", epoch, n))
                _same_batches(z, r, ("zero-copy against resident", epoch, n))
                _same_batches(p, pc, ("no fim", epoch, n))
                assert ("labels" in c) == labels and r["input_ids"].is_cuda
                for k in ("attention_mask", "position_ids", "segment_ids", "cu_seqlens"):
                    assert torch.equal(c[k], pc[k]), k
                moved += int((c["input_ids"] != pc["input_ids"]).sum())
                n += 1
            assert n == cpu.batches_per_epoch
        assert moved > 100
        assert res.state_dict()["fim"] == zc.state_dict()["fim"] == FIM.state() and plain.state_dict()["fim"] is None
    finally:
        for dl in loaders:
            dl.close()
        src.close()
