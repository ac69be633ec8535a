"""Every row launcher (gather / scatter, collate, split, pack, crop) checks its ``RowIndex`` on the host before it
launches anything, and still refuses the dtype pairs it has no kernel for.

The launchers are called through the native module, below the Python wrappers' own checks. Only selectors that
would terminate and stay inside the 5 source rows if a launcher did *not* check them are used here, so a missing
check shows as a test failure (no exception, a written output) and never as a runaway kernel: an unknown mode,
which ``source_row`` treats as the identity, and a Feistel selector whose last two positions (5 and 6) lie past
its domain of 5 but inside its network of 2^(2 * 2) = 16. A cycle walk from outside the domain ends only for some
round keys (a cycle of the network may lie wholly outside it): with ``WALK_KEYS`` the positions 3, 4, 5, 6 reach
rows 2, 1, 4, 2 within four steps, which csrc/kernels/tests/row_index_check.cpp asserts on the host with the same
keys. The selectors that would not terminate are rejected by the same function and covered there alone.
"""

import pytest
import torch

from ddl_amd import _native
from ddl_amd.ops import _dtypes

pytestmark = pytest.mark.gpu

N_SRC, N_OUT, ROW = 5, 4, 8
GUARD = 77
WALK_KEYS = [31, 32, 33, 34, 35, 36]  # kGpuTestKeys of csrc/kernels/tests/row_index_check.cpp
BAD_SELECTORS = {
    "unknown mode": dict(mode=3, idx=0, base=0, keys=[0] * 6, n_domain=1, half_bits=1),
    "positions past the domain": dict(mode=2, idx=0, base=3, keys=WALK_KEYS, n_domain=5, half_bits=2),
}
IDENTITY = dict(mode=0, idx=0, base=0, keys=[0] * 6, n_domain=1, half_bits=1)
U8, F16, BF16, F32 = (_dtypes.code(t) for t in (torch.uint8, torch.float16, torch.bfloat16, torch.float32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dtype):
    return torch.full(shape, GUARD, dtype=dtype, device="cuda")


def _gather(sel, out_dtype=torch.float32, scatter=False):
    src = torch.arange(N_SRC * ROW, dtype=torch.float32, device="cuda").view(N_SRC, ROW)
    out = _guarded((N_SRC if scatter else N_OUT, ROW), out_dtype)
    call = lambda: _native.hip().gather_rows(  # noqa: E731
        dst=out.data_ptr(), out_dt=_dtypes.code(out_dtype), src=src.data_ptr(), in_dt=F32, n_rows=N_OUT,
        row_elems=ROW, scale=[], bias=[], plane=0, scatter=scatter, stream=_stream(), **sel)
    return call, [out], src


def _scatter(sel):
    return _gather(sel, scatter=True)


def _collate(sel, in_dtype=torch.uint8):
    src = torch.arange(N_SRC * 12, device="cuda").to(in_dtype).view(N_SRC, 2, 2, 3)
    out = _guarded((N_OUT, 3, 2, 2), torch.bfloat16)
    call = lambda: _native.hip().collate_hwc_to_chw(  # noqa: E731
        dst=out.data_ptr(), out_dt=BF16, src=src.data_ptr(), in_dt=_dtypes.code(in_dtype), batch=N_OUT, pixels=4,
        channels=3, scale=[], bias=[], stream=_stream(), **sel)
    return call, [out], src


def _split(sel, out_dtype=torch.bfloat16):
    src = torch.arange(N_SRC * ROW, dtype=torch.float32, device="cuda").view(N_SRC, ROW)
    outs = [_guarded((N_OUT, 3), out_dtype), _guarded((N_OUT, 5), out_dtype)]
    call = lambda: _native.hip().split_columns(  # noqa: E731
        dsts=[o.data_ptr() for o in outs], widths=[3, 5], out_dt=_dtypes.code(out_dtype), src=src.data_ptr(),
        in_dt=F32, n_rows=N_OUT, n_values=ROW, stream=_stream(), **sel)
    return call, outs, src


def _pack(sel, out_dtype=torch.bfloat16):
    groups = [torch.ones((N_SRC, 3), dtype=torch.float32, device="cuda"),
              torch.ones((N_SRC, 5), dtype=torch.float32, device="cuda")]
    out = _guarded((N_OUT, ROW), out_dtype)
    call = lambda: _native.hip().pack_columns(  # noqa: E731
        srcs=[g.data_ptr() for g in groups], widths=[3, 5], in_dt=F32, dst=out.data_ptr(),
        out_dt=_dtypes.code(out_dtype), n_rows=N_OUT, n_values=ROW, stream=_stream(), **sel)
    return call, [out], groups


def _crop(sel, in_dtype=torch.uint8, out_dtype=torch.bfloat16, in_w=2, path=0):
    src = (torch.arange(N_SRC * 2 * in_w * 3, device="cuda") % 251).to(in_dtype).view(N_SRC, 2, in_w, 3)
    out, boxes = _guarded((N_OUT, 3, 2, 2), out_dtype), _guarded((N_OUT, 5), torch.int32)
    call = lambda: _native.hip().random_resized_crop(  # noqa: E731
        dst=out.data_ptr(), out_dt=_dtypes.code(out_dtype), src=src.data_ptr(), in_dt=_dtypes.code(in_dtype),
        batch=N_OUT, hwc=True, in_h=2, in_w=in_w, channels=3, out_h=2, out_w=2, seed=1, sample_base=0,
        scale_min=0.08, scale_max=1.0, ratio_min=0.75, ratio_max=4.0 / 3.0, flip_p=0.5, scale=[], bias=[], boxes_out=boxes.data_ptr(), path=path,
        stream=_stream(), **sel)
    return call, [out, boxes], src


def _assert_refused(call, outs, code):
    with pytest.raises(ValueError, match=rf"\(code {code}\)"):
        call()
    torch.cuda.synchronize()
    for o in outs:
        assert (o == GUARD).all(), "a refused launch wrote to its output"


@pytest.mark.parametrize("selector", sorted(BAD_SELECTORS))
@pytest.mark.parametrize("op", [_gather, _scatter, _collate, _split, _pack, _crop])
def test_bad_row_index_is_refused_before_any_launch(op, selector):
    call, outs, _keep = op(BAD_SELECTORS[selector])
    _assert_refused(call, outs, -2)


@pytest.mark.parametrize("op,kwargs,code", [
    (_gather, dict(out_dtype=torch.uint8), -3),     # a conversion into uint8
    (_collate, dict(in_dtype=torch.float16), -1),   # f16 is a gather-only dtype
    (_split, dict(out_dtype=torch.float16), -1),
    (_pack, dict(out_dtype=torch.float16), -1),
    (_crop, dict(in_dtype=torch.float16), -1),
    # the dtypes are checked before anything is launched or planned: no boxes are drawn for an output dtype without
    # a kernel, and it is reported (-1) ahead of a band that does not fit the LDS path (-5, the next case)
    (_crop, dict(out_dtype=torch.float16), -1),
    (_crop, dict(out_dtype=torch.float16, in_w=4000, path=1), -1),
    (_crop, dict(in_w=4000, path=1), -5),
])
def test_unsupported_dtype_pairs_are_still_refused(op, kwargs, code):
    call, outs, _keep = op(IDENTITY, **kwargs)
    _assert_refused(call, outs, code)


@pytest.mark.parametrize("op", [_gather, _scatter, _collate, _split, _pack, _crop])
def test_good_row_index_still_launches(op):
    """The same calls with a selector inside its domain run, so the refusals above are the check's."""
    good = dict(BAD_SELECTORS["positions past the domain"], base=1)  # positions 1 .. 4 of 5
    call, outs, _keep = op(good)
    call()
    torch.cuda.synchronize()
    assert not (outs[0] == GUARD).all()
