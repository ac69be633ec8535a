"""The differential cases of the row and collate ops, written once for any device.

Each ``run_*`` runs the ops of ``ddl_amd.ops`` on tensors of ``dev`` and compares them with the independent
references of ``tests/kernel_refs.py``: on the CPU the ops take the project's ``ref_*`` paths
(tests/test_kernel_refs.py), on the GPU the HIP kernels (tests/test_kernels_matrix_gpu.py).
"""

from __future__ import annotations

import numpy as np
import torch

from ddl_amd import ops
from tests import kernel_refs as R
from tests.kernel_refs import BF16, F32, HOWS, N_SRC, U8

MAX_BLOCKS = (0, 1, 3)


def _kind(exact: bool) -> str:
    return "ints" if exact else "real"


def _guarded(shape, dtype, dev):
    """An ``out=`` that holds none of the result yet: a recycled allocation could hide a store that is skipped."""
    return torch.full(tuple(shape), R.GUARD, dtype=dtype, device=dev)


def _max_blocks(row_elems):
    return MAX_BLOCKS if row_elems >= 2048 else (0,)


# ------------------------------------------------------------ converting gather
def run_gather_cast(row_elems, how, dev, paths=None):
    """Every cast pair without an affine, every grid cap."""
    seed = R.ROW_ELEMS.index(row_elems) * 3 + HOWS.index(how)
    rows = R.rows_of(N_SRC, R.n_gathered(seed), how, seed)
    kw = rows.kw(dev)
    for in_dt in R.IN_DTYPES:
        src = R.make_source(in_dt, (N_SRC, row_elems), "real", seed)
        d = src.to(dev)
        for out_dt in R.OUT_DTYPES:
            if out_dt == in_dt:
                continue
            ref = R.ref_convert(src, rows.rows, out_dt)
            for mb in _max_blocks(row_elems):
                out = ops.gather_rows(d, out=_guarded(ref.shape, out_dt, dev), max_blocks=mb, **kw)
                R.assert_same(out, ref, f"cast {R.name(in_dt)}->{R.name(out_dt)} row={row_elems} {how} mb={mb}")
                if paths is not None:
                    paths.add((R.convert_path(in_dt, out_dt, row_elems, d.data_ptr(), out.data_ptr()), in_dt, out_dt))


def run_gather_affine(row_elems, channels, plane, dev, exact=True, paths=None, case=0):
    """Every pair (the same-dtype ones included) under a per-channel affine, every addressing mode; the grid cap
    rotates with the addressing mode and the case."""
    sc, bi = R.exact_affine(channels) if exact else (None, None)
    for pi, (in_dt, out_dt) in enumerate(R.AFFINE_PAIRS):
        if not exact:
            sc, bi = R.realistic_affine(in_dt)
        src = R.make_source(in_dt, (N_SRC, row_elems), _kind(exact), seed=row_elems % 97 + channels)
        d = src.to(dev)
        for hi, how in enumerate(HOWS):
            seed = row_elems % 89 + 7 * channels + hi + pi
            rows = R.rows_of(N_SRC, R.n_gathered(seed), how, seed)
            mb = _max_blocks(row_elems)[(hi + case + pi) % len(_max_blocks(row_elems))]
            ref = R.ref_convert(src, rows.rows, out_dt, sc, bi, plane)
            out = ops.gather_rows(d, out=_guarded(ref.shape, out_dt, dev), scale=sc, bias=bi, plane=plane,
                                  max_blocks=mb, **rows.kw(dev))
            what = (f"affine {R.name(in_dt)}->{R.name(out_dt)} row={row_elems} ch={channels} plane={plane} {how} "
                    f"mb={mb}")
            if exact:
                R.assert_same(out, ref, what)
            else:
                R.assert_within_ulp(out, ref, 1, what)
            if paths is not None:
                paths.add((R.convert_path(in_dt, out_dt, row_elems, d.data_ptr(), out.data_ptr(), plane), in_dt,
                           out_dt))


# (row_elems, channels, plane): the % channels wrap on a vector kernel, a per-column table, an odd plane
AFFINE_EXTRA = ((2048, 3, 8), (2048, 16, 1), (2049, 3, 683))
# rows of three planes under the realistic affine: flat, one chunk / two u8 chunks, several chunks
REALISTIC_ROW_ELEMS = (3 * 680, 3 * 2736, 3 * 5464)


def run_gather_misaligned(side, dev, paths=None, ptrs=None):
    """A source (``side="src"``) or an ``out=`` (``"out"``) one element off its allocation: long rows that would
    take a vector kernel take the flat one, and nothing outside ``out`` is written."""
    row = R.MISALIGNED_ROW_ELEMS
    sc, bi = R.exact_affine(4)
    for pi, (in_dt, out_dt) in enumerate(R.AFFINE_PAIRS):
        src = R.make_source(in_dt, (N_SRC, row), "ints", seed=pi)
        rows = R.rows_of(N_SRC, R.n_gathered(pi), HOWS[pi % 3], pi)
        d = R.offset_view(src.to(dev)) if side == "src" else src.to(dev)
        for affine in ((sc, bi, row // 4), (None, None, None)):
            if affine[0] is None and in_dt == out_dt:
                continue  # a move: run_moves
            out_buf = out = None
            if side == "out":
                out_buf, out = R.offset_buffer((len(rows), row), out_dt, dev)
            res = ops.gather_rows(d, out=out, out_dtype=out_dt, scale=affine[0], bias=affine[1], plane=affine[2],
                                  **rows.kw(dev))
            ref = R.ref_convert(src, rows.rows, out_dt, *affine)
            R.assert_same(res, ref, f"misaligned {side} {R.name(in_dt)}->{R.name(out_dt)} affine={affine[0] is not None}")
            if out_buf is not None:
                assert res is out
                R.assert_guards(out_buf, 1, f"misaligned out {R.name(in_dt)}->{R.name(out_dt)}")
            if ptrs is not None:
                ptrs.append((d if side == "src" else out).data_ptr())
            if paths is not None:
                paths.add((R.convert_path(in_dt, out_dt, row, d.data_ptr(), res.data_ptr(), affine[2]), in_dt, out_dt))


def run_cast_reshape(dev):
    """``ops.cast`` of a 1-D and a 3-D tensor (reshaped to rows inside)."""
    for shape in ((4099,), (5, 3, 1368)):
        for in_dt, out_dt in R.CAST_PAIRS:
            x = R.make_source(in_dt, shape, "real", seed=len(shape))
            out = ops.cast(x.to(dev), out_dt)
            ref = R._round(x.double(), out_dt)
            R.assert_same(out, ref, f"cast {shape} {R.name(in_dt)}->{R.name(out_dt)}")
    x = R.make_source(U8, (5, 3, 1368), "real", seed=5)
    sc, bi = R.exact_affine(3)
    out = ops.cast(x.to(dev), BF16, scale=sc, bias=bi, plane=1368)
    R.assert_same(out, R.ref_convert(x, torch.arange(5), BF16, sc, bi, 1368), "cast 3-D with an affine")


def run_special_values(kind, dev, paths=None):
    """float32 special values to bf16 / f16 / f32 with no affine, at lane 0, lane 7 and a chunk's last group."""
    row = R.SPECIAL_ROW_ELEMS[kind]
    src, cols = R.special_source(row)
    d = src.to(dev)
    for hi, how in enumerate(HOWS):
        rows = R.rows_of(N_SRC, R.n_gathered(hi + 2), how, hi + 2)
        for out_dt in R.OUT_DTYPES:
            ref = R.ref_convert(src, rows.rows, out_dt)
            out = ops.gather_rows(d, out=_guarded(ref.shape, out_dt, dev), **rows.kw(dev))
            R.assert_same(out, ref, f"special values f32->{R.name(out_dt)} {kind} {how}")
            if paths is not None:
                paths.add((R.convert_path(F32, out_dt, row, d.data_ptr(), out.data_ptr()), F32, out_dt))
    return cols


# ----------------------------------------------------------------------- moves
def run_moves(dtype, row_elems, offsets, dev, units=None):
    """Same-dtype gather and scatter, bit-exact, with the source or the destination ``off`` elements off its
    allocation: the result does not depend on the unit (16 / 4 / 1 bytes) the move ran with."""
    src = R.make_source(dtype, (N_SRC, row_elems), "real", seed=row_elems % 13)
    es = src.element_size()
    for off in offsets:
        for side in (("none",) if off == 0 else ("src", "dst")):
            for hi, how in enumerate(HOWS):
                seed = hi + off
                rows = R.rows_of(N_SRC, R.n_gathered(seed), how, seed)
                what = f"{R.name(dtype)} row={row_elems} off={off} on {side} {how}"
                # gather
                d = R.offset_view(src.to(dev), off) if side == "src" else src.to(dev)
                out_buf, out = None, _guarded((len(rows), row_elems), dtype, dev)
                if side == "dst":
                    out_buf, out = R.offset_buffer((len(rows), row_elems), dtype, dev, off)
                res = ops.gather_rows(d, out=out, max_blocks=(0, 2)[hi % 2], **rows.kw(dev))
                R.assert_same(res, src[rows.rows], "gather " + what)
                if out_buf is not None:
                    R.assert_guards(out_buf, off, "gather " + what)
                if units is not None:
                    units.add((dtype, row_elems * es, R.move_unit(row_elems * es, d.data_ptr(), res.data_ptr())))
            # scatter: a permutation index (repeats would race); rows it does not name keep the sentinel
            n = R.n_gathered(off + row_elems)
            idx = torch.from_numpy(np.random.default_rng(off + row_elems).permutation(N_SRC)[:n].copy())
            upd = src[:n].contiguous()
            u = R.offset_view(upd.to(dev), off) if side == "src" else upd.to(dev)
            if side == "dst":
                dst_buf, dst = R.offset_buffer((N_SRC, row_elems), dtype, dev, off)
            else:
                dst_buf, dst = None, torch.full((N_SRC, row_elems), R.GUARD, dtype=dtype, device=dev)
            ref = torch.full((N_SRC, row_elems), R.GUARD, dtype=dtype)
            ref[idx] = upd
            res = ops.scatter_rows(dst, u, idx.to(dev))
            assert res is dst
            R.assert_same(dst, ref, f"scatter {R.name(dtype)} row={row_elems} off={off} on {side}")
            if dst_buf is not None:
                R.assert_guards(dst_buf, off, "scatter")


# --------------------------------------------------------------------- collate
def run_collate(channels, hw, dev):
    """HWC -> CHW for every dtype pair: no affine, the exact affine (also into an ``out=`` one element off its
    allocation), and the realistic one for three channels; the addressing mode rotates over the combinations."""
    h, w = hw
    k = 0
    for in_dt in R.COLLATE_IN:
        for out_dt in R.COLLATE_OUT:
            affines = [("none", None, None), ("exact", *R.exact_affine(channels))]
            if channels == 3:
                affines.append(("real", *R.realistic_affine(in_dt)))
            for aname, sc, bi in affines:
                src = R.make_source(in_dt, (R.COLLATE_N_SRC, h, w, channels), _kind(aname == "exact"), seed=h * w % 31)
                d = src.to(dev)
                how = HOWS[k % 3]
                k += 1
                rows = R.collate_rows(how, seed=k)
                ref = R.ref_collate(src, rows.rows, out_dt, sc, bi)
                what = f"collate C={channels} hw={hw} {R.name(in_dt)}->{R.name(out_dt)} {aname} {how}"
                out = ops.collate_hwc_to_chw(d, out_dtype=out_dt, scale=sc, bias=bi, **rows.kw(dev))
                assert tuple(out.shape) == (R.COLLATE_BATCH, channels, h, w) and out.is_contiguous()
                if aname == "real":
                    R.assert_within_ulp(out, ref, 1, what)
                else:
                    R.assert_same(out, ref, what)
                if aname == "exact":
                    buf, view = R.offset_buffer(ref.shape, out_dt, dev)
                    res = ops.collate_hwc_to_chw(d, out_dtype=out_dt, scale=sc, bias=bi, out=view, **rows.kw(dev))
                    assert res is view
                    R.assert_same(view, ref, what + " into an offset out=")
                    R.assert_guards(buf, 1, what)


# ------------------------------------------------------------------ split/pack
def run_split_pack(n_rows, n_values, dev):
    case = R.SPLIT_ROWS.index(n_rows) + R.SPLIT_VALUES.index(n_values)
    all_rows = torch.arange(R.SPLIT_N_SRC)
    pairs = [(dt, dt) for dt in R.SPLIT_RAW] + list(R.SPLIT_CONVERT)
    for gi, widths in enumerate(R.split_groups(n_values)):
        how = HOWS[(gi + case) % 3]
        rows = R.split_rows(n_rows, how, seed=case + gi)
        kw = rows.kw(dev)
        for in_dt, out_dt in pairs:
            what = f"rows={n_rows} values={n_values} groups={len(widths)} {R.name(in_dt)}->{R.name(out_dt)} {how}"
            src = R.make_source(in_dt, (R.SPLIT_N_SRC, n_values), "real", seed=n_values % 11)
            # split
            outs = ops.split_columns(src.to(dev), widths, out_dtype=out_dt, **kw)
            refs = R.ref_split(src, rows.rows, widths, out_dt)
            assert len(outs) == len(refs)
            for g, (o, r) in enumerate(zip(outs, refs)):
                assert o.is_contiguous(), f"split {what}: group {g} is not contiguous"
                R.assert_same(o, r, f"split {what} group {g}")
            # pack: the groups of the whole source, gathered and concatenated
            groups = R.ref_split(src, all_rows, widths)
            packed = ops.pack_columns([g.to(dev) for g in groups], out=_guarded((n_rows, n_values), out_dt, dev), **kw)
            R.assert_same(packed, R.ref_pack(groups, rows.rows, out_dt), f"pack {what}")
            # round trip: splitting the packed block gives the gathered (and cast) groups back
            back = ops.split_columns(packed, widths)
            for g, (o, r) in enumerate(zip(back, refs)):
                R.assert_same(o, r, f"split(pack) {what} group {g}")
