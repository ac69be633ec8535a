"""CPU half of the kernel matrix: the ops' ``ref_*`` paths against the independent float64 references.

The GPU suite trusts ``ops.ref_*``; this file checks them (NaNs, ties, channel arithmetic, addressing) with the
case tables of tests/kernel_matrix.py, and proves the tables sound before a GPU sees them: exact affines are
exact, misaligned views are misaligned, and the cases reach every kernel the host dispatch can pick.
"""

import numpy as np
import pytest
import torch

from tests import kernel_matrix as M
from tests import kernel_refs as R
from tests.kernel_refs import BF16, F16, F32, U8

CPU = torch.device("cpu")


# ------------------------------------------------------------------- the rules
def test_assert_same_rules():
    a = torch.tensor([1.0, float("nan"), -0.0, 3.0])
    R.assert_same(a.clone(), a)
    nan2 = a.clone()
    nan2.view(torch.int32)[1] = -1  # another NaN payload and sign
    R.assert_same(nan2, a)
    for bad in (torch.tensor([1.0, 2.0, -0.0, 3.0]), torch.tensor([1.0, float("nan"), 0.0, 3.0]),
                torch.tensor([float("nan"), float("nan"), -0.0, 3.0])):
        with pytest.raises(AssertionError, match="1 of 4 elements differ"):
            R.assert_same(bad, a)
    with pytest.raises(AssertionError):
        R.assert_same(a.double(), a)
    i = torch.arange(12, dtype=torch.int64).view(3, 4)
    R.assert_same(i.clone(), i)
    j = i.clone()
    j[2, 1] += 1
    with pytest.raises(AssertionError, match=r"row 2, elem 1"):
        R.assert_same(j, i)


def test_assert_within_ulp_rules():
    for dt in (BF16, F16, F32):
        x = torch.tensor([1.0, -1.0, 0.0, 100.0, 2.0 ** -10], dtype=dt)
        up = torch.nextafter(x.float(), torch.tensor(float("inf"))).to(dt) if dt == F32 else \
            (x.view(torch.int16) + torch.tensor([1, -1, 1, 1, 1], dtype=torch.int16)).view(dt)
        R.assert_within_ulp(up, x, 1)
        with pytest.raises(AssertionError):
            R.assert_within_ulp(up, x, 0)
    x = torch.tensor([1.0])
    with pytest.raises(AssertionError):
        R.assert_within_ulp(x + 3 * 2.0 ** -23, x, 1)
    R.assert_within_ulp(torch.tensor([-0.0]), torch.tensor([0.0]), 0)


def test_rows_of():
    for seed in range(6):
        n = R.n_gathered(seed)
        assert 5 <= n <= 9
        ident, index, perm = (R.rows_of(R.N_SRC, n, how, seed) for how in R.HOWS)
        assert ident.rows.tolist() == list(range(3, 3 + n)) and ident.kw() == dict(base=3, n_rows=n)
        idx = index.rows.tolist()
        assert len(set(idx)) < len(idx) and idx != sorted(idx) and 0 in idx and R.N_SRC - 1 in idx
        assert perm.rows.tolist() == perm.perm.numpy_eval(np.arange(2, 2 + n)).tolist()
        assert len(set(perm.rows.tolist())) == n


def test_reference_roundings():
    """The references' own edge behaviour, against hand-computed bit patterns."""
    src = torch.tensor([0x3F808000, 0x3F818000, 0x3F808001, 0x7F7FFFFF, 0x007FFFFF, 0x00000001, 0x7F800001],
                       dtype=torch.int64).to(torch.int32).view(F32).reshape(1, -1)
    out = R.ref_convert(src, torch.tensor([0]), BF16).view(torch.int16).reshape(-1)
    assert [v & 0xFFFF for v in out.tolist()][:6] == [0x3F80, 0x3F82, 0x3F81, 0x7F80, 0x0080, 0x0000]
    assert torch.isnan(R.ref_convert(src, torch.tensor([0]), BF16).float()[0, 6])
    h = torch.tensor([[65504.0, 65519.99, 65520.0, 2.0 ** -24, 2.0 ** -25, float(np.nextafter(np.float32(2.0 ** -25),
                                                                                               np.float32(1)))]])
    out = R.ref_convert(h, torch.tensor([0]), F16).view(torch.int16).reshape(-1)
    assert [v & 0xFFFF for v in out.tolist()] == [0x7BFF, 0x7BFF, 0x7C00, 0x0001, 0x0000, 0x0001]
    # channel arithmetic: plane 2, 3 channels, 8 elements -> channels 0 0 1 1 2 2 0 0
    x = torch.ones(1, 8)
    out = R.ref_convert(x, torch.tensor([0]), F32, [1, 2, 4], [0, 0, 0], 2)
    assert out.reshape(-1).tolist() == [1, 1, 2, 2, 4, 4, 1, 1]
    img = torch.arange(2 * 3 * 2, dtype=F32).view(1, 2, 3, 2)  # [N, H, W, C]
    out = R.ref_collate(img, torch.tensor([0]), F32, [1, -1], [0, 100])
    assert out.shape == (1, 2, 2, 3) and out[0, 0].reshape(-1).tolist() == [0, 2, 4, 6, 8, 10]
    assert out[0, 1].reshape(-1).tolist() == [99, 97, 95, 93, 91, 89]


# --------------------------------------------------------- soundness of tables
def test_exact_affines_are_exact():
    for in_dt in R.IN_DTYPES:
        for ch in R.AFFINE_CHANNELS:
            sc, bi = R.exact_affine(ch)
            assert len(set(zip(sc, bi))) == ch  # distinct per channel: a mix-up changes bits
            for row in (7, 2048):
                src = R.make_source(in_dt, (R.N_SRC, row), "ints")
                assert R.affine_is_exact(src, sc, bi, R.plane_for(row, ch))
    for in_dt in R.COLLATE_IN:
        for ch in R.COLLATE_CHANNELS:
            src = R.make_source(in_dt, (R.COLLATE_N_SRC, 8, 257, ch), "ints")
            assert R.affine_is_exact(src, *R.exact_affine(ch), None)
    # the whole input range, not only the sampled sources
    for ch in range(16):
        sc, bi = R.exact_affine(16)
        for x in (torch.arange(256), torch.arange(-64, 64)):
            y = x.double() * sc[ch] + bi[ch]
            assert torch.equal(y.float().double(), y)
    # and the realistic affine is not (else its cases would test nothing beyond the exact ones)
    src = R.make_source(U8, (R.N_SRC, 2040), "real")
    assert not R.affine_is_exact(src, *R.realistic_affine(U8), 680)


def test_plane_for():
    for row in R.ROW_ELEMS:
        for ch in R.AFFINE_CHANNELS:
            p = R.plane_for(row, ch)
            assert p >= 1 and p * ch <= max(row, ch)
            assert p * ch == row or row % ch
    assert R.plane_for(2048, 3) == 680 and R.plane_for(7, 3) == 2 and R.plane_for(1, 16) == 1


def test_special_value_placement():
    for kind, row in R.SPECIAL_ROW_ELEMS.items():
        src, cols = R.special_source(row)
        bits = src.view(torch.int32)
        assert len(cols) == len(R.SPECIAL_F32_BITS) >= 28
        for b, (c0, c7, cl) in zip(R.SPECIAL_F32_BITS, cols):
            assert c0 % 8 == 0 and c7 % 8 == 7 and (cl // 8 + 1) * 8 % R.SPECIAL_CHUNK == 0
            for c in (c0, c7, cl):
                assert all((v & 0xFFFFFFFF) == b for v in bits[:, c].tolist())
        assert int(torch.isnan(src).sum()) == 6 * 3 * R.N_SRC


def test_move_table():
    cases = R.move_cases()
    assert {dt for dt, _, _ in cases} == set(R.MOVE_DTYPES)
    for dt, row_elems, offs in cases:
        es = torch.empty((), dtype=dt).element_size()
        assert offs[0] == 0 and ((row_elems * es) % 16 != 0) == (len(offs) == 1)
    assert any(dt == torch.int64 for dt, _, _ in cases)


# ------------------------------------------------------ the ops' CPU references
PATHS: set = set()
MISALIGNED_PTRS: list = []
UNITS: set = set()


@pytest.mark.parametrize("how", R.HOWS)
@pytest.mark.parametrize("row_elems", R.ROW_ELEMS)
def test_ref_gather_cast(row_elems, how):
    M.run_gather_cast(row_elems, how, CPU, PATHS)


@pytest.mark.parametrize("channels", R.AFFINE_CHANNELS)
@pytest.mark.parametrize("row_elems", R.ROW_ELEMS)
def test_ref_gather_exact_affine(row_elems, channels):
    M.run_gather_affine(row_elems, channels, R.plane_for(row_elems, channels), CPU, paths=PATHS, case=channels)


@pytest.mark.parametrize("row_elems,channels,plane", M.AFFINE_EXTRA)
def test_ref_gather_affine_wrap_table_and_odd_plane(row_elems, channels, plane):
    M.run_gather_affine(row_elems, channels, plane, CPU, paths=PATHS)


@pytest.mark.parametrize("row_elems", M.REALISTIC_ROW_ELEMS)
def test_ref_gather_realistic_affine(row_elems):
    M.run_gather_affine(row_elems, 3, row_elems // 3, CPU, exact=False, paths=PATHS)


@pytest.mark.parametrize("side", ["src", "out"])
def test_ref_gather_misaligned(side):
    M.run_gather_misaligned(side, CPU, PATHS, MISALIGNED_PTRS)


def test_ref_cast_reshape():
    M.run_cast_reshape(CPU)


@pytest.mark.parametrize("kind", ["flat", "chunked"])
def test_ref_special_values(kind):
    M.run_special_values(kind, CPU, PATHS)


@pytest.mark.parametrize("dtype,row_elems,offsets", R.move_cases(),
                         ids=lambda v: R.name(v) if isinstance(v, torch.dtype) else None)
def test_ref_moves(dtype, row_elems, offsets):
    M.run_moves(dtype, row_elems, offsets, CPU, UNITS)


def test_tables_cover_every_dispatch_path():
    """Runs after the cases above (file order): what they recorded through the mirror of the host dispatch.
    CPU allocations are 64-byte aligned like the GPU's, so the recorded paths are the GPU's."""
    if not PATHS or not UNITS or not MISALIGNED_PTRS:  # selected alone: run the cases here
        for row_elems in R.ROW_ELEMS:
            M.run_gather_cast(row_elems, "identity", CPU, PATHS)
            for ch in R.AFFINE_CHANNELS:
                M.run_gather_affine(row_elems, ch, R.plane_for(row_elems, ch), CPU, paths=PATHS)
        for side in ("src", "out"):
            M.run_gather_misaligned(side, CPU, PATHS, MISALIGNED_PTRS)
        for case in R.move_cases():
            M.run_moves(*case, CPU, UNITS)
    assert all(p % 16 != 0 for p in MISALIGNED_PTRS), "a misaligned view is 16-byte aligned"
    for in_dt, out_dt in R.AFFINE_PAIRS:
        want = {"flat", "u8_chunked" if in_dt == U8 else "chunked"}  # u8 sources have their own chunked kernel
        got = {p for p, i, o in PATHS if (i, o) == (in_dt, out_dt)}
        assert want <= got, f"{R.name(in_dt)}->{R.name(out_dt)}: paths {sorted(want - got)} never reached"
    assert {p for p, _, _ in PATHS} >= {"flat", "chunked", "u8_chunked"}
    for dt in R.MOVE_DTYPES:
        units = {u for d, _, u in UNITS if d == dt}
        assert units >= ({16, 4, 1} if dt in (U8, F16) else {16, 4}), R.name(dt)
    # a 16-byte row size takes the narrower units through a misaligned base alone
    for rb in (16 * 255, 16 * 1025):
        assert {u for d, b, u in UNITS if d == U8 and b == rb} == {16, 4, 1}


def test_dispatch_mirror():
    al, off = 4096, 4096 + 2
    assert R.convert_path(F32, BF16, 2048, al, al) == "chunked"
    assert R.convert_path(F32, BF16, 2040, al, al) == "flat"
    assert R.convert_path(F32, BF16, 2049, al, al) == "flat"
    assert R.convert_path(F32, BF16, 8192, off, al) == "flat" == R.convert_path(F32, BF16, 8192, al, off)
    assert R.convert_path(U8, BF16, 16392, al, al) == "u8_chunked"
    assert R.convert_path(U8, F32, 2048, al, al, plane=683) == "flat"
    assert R.convert_path(F32, F32, 2048, al, al) == "move" and R.convert_path(F32, F32, 2048, al, al, 8) == "chunked"
    assert R.move_unit(4096, al, al) == 16 and R.move_unit(4096, al + 4, al) == 4 and R.move_unit(4096, al, al + 1) == 1
    assert R.move_unit(1020, al, al) == 4 and R.move_unit(1021, al, al) == 1


@pytest.mark.parametrize("hw", R.COLLATE_HW, ids=lambda hw: f"{hw[0] * hw[1]}px")
@pytest.mark.parametrize("channels", R.COLLATE_CHANNELS)
def test_ref_collate(channels, hw):
    M.run_collate(channels, hw, CPU)


@pytest.mark.parametrize("n_values", R.SPLIT_VALUES)
@pytest.mark.parametrize("n_rows", R.SPLIT_ROWS)
def test_ref_split_pack(n_rows, n_values):
    M.run_split_pack(n_rows, n_values, CPU)


def test_split_groups_table():
    assert R.split_groups(1) == [(1,)] and R.split_groups(2) == [(2,), (1, 1)]
    g = R.split_groups(257)
    assert len(g) == 3 and len(g[2]) == 8 and all(sum(w) == 257 for w in g)
