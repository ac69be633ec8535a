"""The ``RowIndex`` selectors of the resident loaders: ``ops.row_selector`` gives the dicts the loaders used to
write by hand, and the loaders' one epoch-keyed cache stays bounded."""

import numpy as np
import pytest

import ddl_amd
from ddl_amd import ops
from ddl_amd.models.tokens import SharedTokenSource
from ddl_amd.permutation import FeistelPermutation
from ddl_amd.types import DDLEnv

GB, S = 4, 8


def _by_hand(perm) -> dict:
    """The selector as the loaders spelled it out, at base 0."""
    if perm is not None:
        return dict(mode=2, idx=0, base=0, **perm.device_args())
    return dict(mode=0, idx=0, base=0, keys=[0] * 6, n_domain=1, half_bits=1)


@pytest.fixture(scope="module")
def source():
    src = SharedTokenSource.synthetic(f"ddl_amd_cr_{np.random.randint(1 << 30)}", 64, 1, 40, seed=2, vocab=65536,
                                      token_dtype="uint16")
    yield src
    src.close()


@pytest.mark.parametrize("shuffle", [True, False])
def test_row_selector_gives_the_hand_written_dicts(source, shuffle):
    stream = ddl_amd.ResidentTokenStreamLoader(source, GB, S, DDLEnv(), device="cpu", seed=7, shuffle=shuffle,
                                               shuffle_rows=True)
    docs = ddl_amd.ResidentTokenLoader(source, GB, S, "pack", DDLEnv(), device="cpu", seed=7, plan="device")
    assert (docs._perm(0) is not None) and stream.order.shuffle is shuffle
    try:
        for e in range(10):
            perm = FeistelPermutation(source.n, 7, e) if shuffle else None
            want = _by_hand(perm)
            assert ops.row_selector(None, perm, 0) == want
            assert (want["mode"], len(want["keys"])) == (2 if shuffle else 0, 6)
            got = stream._selector(e)
            assert got == want and list(got) == list(want) and stream._selector(e) is got  # cached
            rows = _by_hand(FeistelPermutation(stream.order.n_samples, stream.row_seed, e))
            assert stream._selector(e, stream._row_perm) == rows and rows["n_domain"] == stream.order.n_samples
            # the sequence-batched loader's order always shuffles; a step sets its own base
            want_docs = _by_hand(docs.order.perm(e))
            assert dict(docs._selector(e), base=5 + e) == dict(want_docs, base=5 + e)
            assert len(stream._selectors) <= 9 and len(docs._selectors) <= 9
        assert len(docs._selectors) == 1 and len(stream._selectors) <= 9  # cleared when more than eight
    finally:
        stream.close()
        docs.close()


def test_selector_cache_holds_nine_entries_after_ten_epochs(source):
    dl = ddl_amd.ResidentTokenLoader(source, GB, S, "pad", DDLEnv(), device="cpu", seed=1, plan="device")
    try:
        sizes = []
        for e in range(10):
            dl._selector(e)
            sizes.append(len(dl._selectors))
        assert sizes == [1, 2, 3, 4, 5, 6, 7, 8, 9, 1]  # today's rule: clear when more than eight are held
        assert max(sizes) <= 9 and dl._selector(9) == _by_hand(dl.order.perm(9))
    finally:
        dl.close()
