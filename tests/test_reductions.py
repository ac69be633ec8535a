"""CPU paths and host twins of the reduction and owner-bucketing ops against the independent references of
``tests/reduction_refs.py``: ``ops.column_stats`` on CPU tensors, ``owner_counts`` / ``owner_maps`` of the native
runtime. The HIP kernels run through the same tables in ``tests/test_reductions_gpu.py`` and
``tests/test_bucketing_gpu.py``."""

import numpy as np
import pytest
import torch

from ddl_amd import _native, ops
from ddl_amd.permutation import FeistelPermutation
from tests import reduction_refs as R


@pytest.mark.parametrize("offset,sd", R.RANDOM_KINDS[:4])
def test_column_stats_cpu_offset_columns(offset, sd):
    """[20000, 9] of offset + sd * randn: a float32 ``sumsq/n - mean^2`` is off by 7 %, 6 % and 300 % in std at
    1000/1, 100/0.1 and 1e4/1 (and fine at 3/1); the float64 form meets the suite's bounds."""
    x = R.offset_table(offset, sd)
    R.check_column_stats(ops.column_stats(torch.tensor(x)), R.ref_column_stats(x), [(offset, sd)] * x.shape[1])


@pytest.mark.parametrize("rows,cols", [(1, 9), (3, 9), (7777, 9), (4096, 1), (999, 300)])
def test_column_stats_cpu_value_cases(rows, cols):
    """Every kind of column of the GPU suite (offset columns, constants, one-signed columns, a lone value, huge
    values) through the CPU path, with the same bounds."""
    for start in R.kind_starts(cols):
        x = R.stats_table(rows, cols, start)
        s = ops.column_stats(torch.tensor(x))
        assert set(s) == {"sum", "sumsq", "min", "max", "mean", "std"}
        assert all(v.dtype == torch.float32 and v.shape == (cols,) for v in s.values())
        R.check_column_stats(s, R.stats_ref(rows, cols, start), [R.column_kind(j, start) for j in range(cols)])


def test_column_stats_sum_and_sumsq_are_the_rounded_totals():
    x = R.stats_table(7777, 9, 0)
    s = ops.column_stats(torch.tensor(x))
    d = x.astype(np.float64)
    np.testing.assert_allclose(s["sum"].numpy(), d.sum(0), rtol=1e-6)
    np.testing.assert_allclose(s["sumsq"].numpy(), (d * d).sum(0), rtol=1e-6)


def test_ref_column_stats_ulp32():
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(-1000.0) == 2.0 ** -14 and R.ulp32(1.5e4) == 2.0 ** -10
    assert R.ulp32(0.0) > 0


@pytest.mark.parametrize("n,gb,world", R.BUCKET_CASES)
def test_owner_counts_and_maps_match_numpy(n, gb, world):
    """The host twins of the bucketing kernels (``owner_counts``: the split sizes of the all-to-all;
    ``owner_maps``: the CPU rehearsal's send list and receive map) for every rank and the first two batches."""
    rt = _native.runtime()
    lb, shard, batches = R.bucket_geometry(n, gb, world)
    assert batches >= 1
    for g in range(batches):
        px = FeistelPermutation(n, R.BUCKET_SEED, g)
        sent = 0
        for rank in range(world):
            ref_send, ref_inv, ref_sc, ref_rc = R.ref_owner_maps(px, n, g, gb, world, rank)
            sc, rc = rt.owner_counts(px.keys, px.half_bits, n, g * gb, gb, lb, shard, world, rank)
            assert list(sc) == ref_sc.tolist() and list(rc) == ref_rc.tolist()
            assert sum(rc) == lb
            send, inv = rt.owner_maps(px.keys, px.half_bits, n, g * gb, gb, lb, shard, world, rank, rank * shard)
            assert send.dtype == inv.dtype == np.int64
            assert np.array_equal(send, ref_send) and len(send) == sum(sc)
            assert np.array_equal(inv, ref_inv)
            assert np.array_equal(np.sort(inv), np.arange(lb))
            sent += sum(sc)
        assert sent == gb


def test_ref_owner_maps_on_a_hand_case():
    """The oracle itself, on an order small enough to check by hand."""

    class Order:
        def numpy_eval(self, pos):
            return np.array([5, 0, 3, 4, 1, 2, 7, 6])[pos]

    # n 8, world 2: shard 4, lb 2; batch 0 = positions 0..3 -> samples 5 0 3 4, owners 1 0 0 1
    send, inv, sc, rc = R.ref_owner_maps(Order(), 8, 0, 4, 2, 0)
    assert send.tolist() == [0, 3] and sc.tolist() == [1, 1]  # samples 0 (to rank 0) and 3 (to rank 1)
    assert inv.tolist() == [1, 0] and rc.tolist() == [1, 1]    # slice owners 1 0: from rank 0 first
    send, inv, sc, rc = R.ref_owner_maps(Order(), 8, 0, 4, 2, 1)
    assert send.tolist() == [1, 0] and sc.tolist() == [1, 1]  # samples 5 and 4, shard-local
    assert inv.tolist() == [0, 1] and rc.tolist() == [1, 1]    # slice owners 0 1
