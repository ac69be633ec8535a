"""One corpus replica in HBM under every resident loader format at once: counted per holder, released in any
order, gone with the last one."""

import numpy as np
import pytest
import torch

import ddl_amd
from ddl_amd import corpus_replica, zerocopy
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.types import DDLEnv

pytestmark = pytest.mark.gpu

GB, S = 4, 8


def _same(a: dict, b: dict) -> None:
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


def test_four_loaders_share_one_replica_and_release_it_in_any_order():
    src = SharedTokenSource.synthetic(f"ddl_amd_crg_{np.random.randint(1 << 30)}", 64, 1, 40, seed=2, vocab=65536,
                                      token_dtype="uint16")
    try:
        assert not corpus_replica.REPLICAS and not zerocopy._SHARED_REGS
        makers = [
            lambda dev: ddl_amd.ResidentTokenLoader(src, GB, S, "pack", DDLEnv(), device=dev, seed=3, plan="host"),
            lambda dev: ddl_amd.ResidentTokenLoader(src, GB, S, "pack", DDLEnv(), device=dev, seed=3, plan="device"),
            lambda dev: ddl_amd.ResidentTokenStreamLoader(src, GB, S, DDLEnv(), device=dev, seed=3),
            lambda dev: ddl_amd.ResidentTokenStreamLoader(src, GB, S, DDLEnv(), device=dev, seed=3,
                                                          shuffle_rows=True),
        ]
        loaders = [make("cuda") for make in makers]
        assert [dl.replica_shared for dl in loaders] == [False, True, True, True]
        (key, rep), = corpus_replica.REPLICAS.items()
        assert rep.users == 4 and all(dl._replica is rep for dl in loaders)
        assert {dl.replica_ptr for dl in loaders} == {rep.hbm.data_ptr()}
        assert {dl.load_s for dl in loaders} == {rep.load_s}
        # one offsets tensor in HBM for the three loaders that plan on the device
        offs = rep.offsets_dev
        assert offs is not None and offs.is_cuda and torch.equal(offs.cpu(), src.offsets.tensor().view(-1))
        assert all(dl._replica.offsets_dev.data_ptr() == offs.data_ptr() for dl in loaders[1:])
        for dl, make in zip(loaders, makers):
            twin = make("cpu")
            it, ref = iter(dl), iter(twin)
            for _ in range(2):
                _same(next(it), next(ref))
            del it, ref
            twin.close()
        del rep, offs
        for left, i in zip((3, 2, 1), (2, 0, 3)):  # not the order they were opened in
            loaders[i].close()
            assert loaders[i].replica_ptr is None and corpus_replica.REPLICAS[key].users == left
            loaders[i].close()  # a holder releases once
            assert corpus_replica.REPLICAS[key].users == left
        assert loaders[1].replica_ptr is not None
        assert next(iter(loaders[1]))["input_ids"].is_cuda  # the last holder still reads the replica
        loaders[1].close()
        assert not corpus_replica.REPLICAS and not zerocopy._SHARED_REGS
        assert all(dl.replica_ptr is None for dl in loaders)
    finally:
        src.close()
