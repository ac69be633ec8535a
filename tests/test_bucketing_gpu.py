"""bucket_send / bucket_recv (csrc/kernels/bucket.hip) against the numpy oracle of ``tests/reduction_refs.py``
and the host twin ``owner_maps``: slices longer than one 1024-position chunk (the per-source running count that
bucket_recv carries from chunk to chunk), partial chunks, world 1, and ranks that own nothing."""

import numpy as np
import pytest
import torch

from ddl_amd import _native
from ddl_amd.permutation import FeistelPermutation
from tests import reduction_refs as R

pytestmark = pytest.mark.gpu

GUARD = -(0x5A5A5A5A5A5A5A5A)
TAIL = 8  # guard elements past each output


@pytest.mark.parametrize("n,gb,world", R.BUCKET_CASES)
def test_bucketing_kernels_every_rank(n, gb, world):
    """Every rank, the first two global batches: the send list equals the oracle and the slots past it keep the
    guard; the receive map equals the oracle and is a permutation of the slice; the counts add up; the device
    maps equal the host twin's element for element."""
    hip, rt = _native.hip(), _native.runtime()
    dev = torch.device("cuda", torch.cuda.current_device())
    lb, shard, batches = R.bucket_geometry(n, gb, world)
    st = torch.cuda.current_stream().cuda_stream
    assert batches >= 1
    for g in range(batches):
        px = FeistelPermutation(n, R.BUCKET_SEED, g)
        sent = 0
        for rank in range(world):
            ref_send, ref_inv, ref_sc, ref_rc = R.ref_owner_maps(px, n, g, gb, world, rank)
            sc, rc = rt.owner_counts(px.keys, px.half_bits, n, g * gb, gb, lb, shard, world, rank)
            assert list(sc) == ref_sc.tolist() and list(rc) == ref_rc.tolist() and sum(rc) == lb
            n_send = sum(sc)
            sent += n_send
            send = torch.full((gb + TAIL,), GUARD, dtype=torch.int64, device=dev)
            inv = torch.full((lb + TAIL,), GUARD, dtype=torch.int64, device=dev)
            hip.bucket_send(px.keys, n, px.half_bits, g * gb, gb, shard, rank * shard, rank, world, send.data_ptr(),
                            st)
            offs = np.concatenate([[0], np.cumsum(rc)[:-1]]).tolist()
            hip.bucket_recv(px.keys, n, px.half_bits, g * gb + rank * lb, lb, shard, world, offs, inv.data_ptr(), st)
            send, inv = send.cpu().numpy(), inv.cpu().numpy()
            where = f"batch {g} rank {rank}"
            assert n_send == len(ref_send), where
            assert np.array_equal(send[:n_send], ref_send), where
            assert (send[n_send:] == GUARD).all(), where
            assert np.array_equal(inv[:lb], ref_inv), where
            assert (inv[lb:] == GUARD).all(), where
            assert np.array_equal(np.sort(inv[:lb]), np.arange(lb)), where
            h_send, h_inv = rt.owner_maps(px.keys, px.half_bits, n, g * gb, gb, lb, shard, world, rank, rank * shard)
            assert np.array_equal(send[:n_send], h_send) and np.array_equal(inv[:lb], h_inv), where
        assert sent == gb
