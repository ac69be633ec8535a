"""CPU tests of the crop-and-resize references and tables of tests/augment_refs.py: the resampler against
``F.interpolate``, the comparator against deliberately wrong resamplers, the ambiguity share of every box case, and
the coverage of the kernel's dispatch paths by the shape lists that tests/test_augment_matrix_gpu.py runs."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import augment_refs as A
from tests import kernel_refs as R
from tests.kernel_refs import BF16, F32, U8

ALL_PIXEL_CASES = A.CROP_CASES + A.MOAT_CASES


# ------------------------------------------------------------------ ref_resample
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_ref_resample_matches_interpolate(layout):
    """Up- and downsampling, 1x1, 1xk and kx1 crops, crops at the image's corners, flipped and not. Both sides
    are float64; they differ by the rounding of the coordinate (a few float64 ulps of a coordinate below 2^6 here)
    times the spread of the pixels, and of three interpolations: 2^-53 * (8 * 64 + 16) * max |pixel| is generous."""
    H, W, C = 23, 31, 3
    src = A.images(F32, layout, C, (H, W), "noise", seed=3)
    boxes = [(0, 0, H, W, 0), (0, 0, H, W, 1), (5, 7, 1, 1, 0), (22, 30, 1, 1, 1), (3, 4, 1, 9, 1), (2, 30, 11, 1, 0),
             (10, 12, 13, 19, 1), (0, 24, 4, 7, 0), (19, 0, 4, 5, 1), (6, 6, 2, 3, 0), (1, 2, 20, 28, 1)]
    rows = np.arange(len(boxes)) % A.N_SRC
    sc, bi = R.exact_affine(C)
    for size in ((8, 8), (5, 13), (40, 37), (23, 31), (1, 1), (46, 62)):
        ref = A.ref_resample(src, rows, boxes, size, layout, F32, sc, bi)
        x = src[torch.as_tensor(rows)]
        x = (x.movedim(-1, 1) if layout == "hwc" else x).double()
        tol = 2.0 ** -53 * (8 * 64 + 16) * float(x.abs().max())
        for i, (y0, x0, h, w, flip) in enumerate(boxes):
            r = F.interpolate(x[i:i + 1, :, y0:y0 + h, x0:x0 + w], size=size, mode="bilinear", align_corners=False)[0]
            if flip:
                r = r.flip(-1)
            r = r * torch.tensor(sc, dtype=torch.float64).view(C, 1, 1) + torch.tensor(bi).double().view(C, 1, 1)
            d = float((r - ref.value[i]).abs().max())
            assert d <= tol, f"{layout} size {size} box {boxes[i]}: {d} > {tol}"
        assert ref.out.dtype == F32 and torch.equal(ref.out, ref.value.float())
        A.assert_resampled(ref.out, ref, f"the reference's own float32 rounding, size {size}")


def test_ref_resample_out_dtype_and_no_affine():
    src = A.images(U8, "chw", 1, (6, 8), "ints")
    ref = A.ref_resample(src, [0, 1], [(0, 0, 6, 8, 0), (1, 1, 4, 6, 1)], (3, 4), "chw", BF16)
    assert ref.out.dtype == BF16 and torch.equal(ref.out, ref.value.float().to(BF16))
    assert float(ref.value[0, 0, 0, 0]) == float(src[0, 0, :2, :2].double().mean())  # weights 1/2 both ways


# --------------------------------------------------------- the comparator is sharp
def _case_inputs(case, kind):
    rows = A.case_rows(case)
    boxes, amb = A.case_boxes(case, rows)
    src = A.images(case.in_dtype, case.layout, case.channels, case.in_hw, kind, case.seed)
    sc, bi, _, _ = A.affine_of(case.channels, case.in_dtype)
    return src, rows, boxes, amb, sc, bi


def _observable(mutation, case, boxes):
    """Whether a mutant can differ from the reference on these boxes at all."""
    b = boxes.numpy()
    if mutation in ("plane_next", "plane_prev", "affine_next"):
        return case.channels >= 2
    if mutation == "no_flip":
        return bool(b[:, 4].any())
    if mutation == "no_clamp_x":  # the edge tap has a non-zero weight only when upsampling
        return bool((b[:, 3] < case.out_hw[1]).any())
    if mutation == "no_clamp_y":
        return bool((b[:, 2] < case.out_hw[0]).any())
    return True


@pytest.mark.parametrize("kind", ["ramp", "noise"])
@pytest.mark.parametrize("case", A.CROP_CASES, ids=lambda c: c.id)
def test_comparator_rejects_every_mutant(case, kind):
    """On the GPU matrix's own inputs: taps shifted by one pixel in x / y, the neighbour not clamped at the right /
    bottom edge, the flip ignored, the +0.5 dropped, channel c reading plane c +- 1, the affine of the wrong
    channel. Each mutant's float32 output must be refused by ``assert_resampled``; the unmutated one accepted."""
    src, rows, boxes, _, sc, bi = _case_inputs(case, kind)
    args = (src, rows.rows, boxes, case.out_hw, case.layout, F32, sc, bi)
    ref = A.ref_resample(*args)
    A.assert_resampled(ref.out, ref, case.id)
    for mutation in A.MUTATIONS:
        if not _observable(mutation, case, boxes):
            continue
        mutant = A._resample(*args, mutate=mutation)
        with pytest.raises(AssertionError):
            A.assert_resampled(mutant.out, ref, f"{case.id} {mutation}")
        with pytest.raises(AssertionError):  # and in bfloat16, through the bit rule
            A.assert_bf16_of(mutant.out.to(BF16), ref.out, f"{case.id} {mutation}")


def test_every_mutation_is_observable_in_several_cases():
    seen = {m: 0 for m in A.MUTATIONS}
    for case in A.CROP_CASES:
        boxes, _ = A.case_boxes(case, A.case_rows(case))
        for m in A.MUTATIONS:
            seen[m] += _observable(m, case, boxes)
    assert all(n >= 3 for n in seen.values()), seen
    assert all(seen[m] == len(A.CROP_CASES) for m in ("shift_x", "shift_y", "no_half", "no_flip")), seen


# -------------------------------------------------------------------- ref_boxes
def test_unit_uniform_is_a_24_bit_fraction():
    u = A.unit_uniform(5, np.arange(1000, dtype=np.uint64), 3)
    assert u.min() >= 0 and u.max() < 1 and np.array_equal(u * 2 ** 24, np.rint(u * 2 ** 24))
    assert 0.45 < u.mean() < 0.55
    # splitmix64's published first output for state 0: mix64(0 + golden gamma)
    assert int(A.mix64(np.array([0x9E3779B97F4A7C15], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("case", A.BOX_CASES, ids=lambda c: c.id)
def test_box_cases_stay_under_the_ambiguity_cap(case):
    H, W = case.in_hw
    boxes, amb = A.ref_boxes(np.arange(case.n), case.in_hw, seed=case.seed, scale=case.scale, ratio=case.ratio)
    share = float(amb.double().mean())
    print(f"{case.id}: ambiguous share {share:.4%}")
    assert share <= A.MAX_AMBIGUOUS
    y, x, h, w, flip = boxes.long().unbind(1)
    assert bool(((y >= 0) & (x >= 0) & (h >= 1) & (w >= 1) & (y + h <= H) & (x + w <= W)).all())
    assert 0.45 < float(flip.double().mean()) < 0.55
    rmin, rmax = case.ratio
    centre = None
    if W / H > rmax:
        fw = min(W, max(1, round(H * rmax)))
        centre = ((H - H) // 2, (W - fw) // 2, H, fw)
    elif W / H < rmin:
        fh = min(H, max(1, round(W / rmin)))
        centre = ((H - fh) // 2, 0, fh, W)
    if case.expect == "fallback":  # no attempt can fit: every sample takes the centre crop of its branch
        assert centre is not None and bool((boxes[:, :4] == torch.tensor(centre, dtype=torch.int32)).all())
    elif case.expect == "some-fallback":
        n_fb = int((boxes[:, :4] == torch.tensor(centre, dtype=torch.int32)).all(1).sum())
        assert 0.02 * case.n < n_fb < 0.98 * case.n, n_fb
    elif case.expect == "1x1":
        assert bool(((h == 1) & (w == 1)).all()) and len(set(zip(y.tolist(), x.tolist()))) > 500
    else:
        assert len(set(map(tuple, boxes[:, :4].tolist()))) > 0.9 * case.n


def test_fallback_branches_are_distinct():
    wide = next(c for c in A.BOX_CASES if c.id.startswith("fallback-wide"))
    tall = next(c for c in A.BOX_CASES if c.id.startswith("fallback-tall"))
    assert wide.in_hw[1] / wide.in_hw[0] > wide.ratio[1] and tall.in_hw[1] / tall.in_hw[0] < tall.ratio[0]
    for c, v in ((wide, wide.in_hw[0] * wide.ratio[1]), (tall, tall.in_hw[1] / tall.ratio[0])):
        assert abs(v - np.floor(v) - 0.5) > 0.1  # rint of the fallback side is nowhere near a tie


@pytest.mark.parametrize("case", ALL_PIXEL_CASES, ids=lambda c: c.id)
def test_pixel_cases_have_no_ambiguous_box(case):
    """8 images: the 2 % cap allows none to be dropped."""
    boxes, amb = A.case_boxes(case, A.case_rows(case))
    assert float(amb.double().mean()) <= A.MAX_AMBIGUOUS
    assert bool(boxes[:, 4].any()) and not bool(boxes[:, 4].all())  # flipped and unflipped images in every case


def test_ref_boxes_keys():
    kw = dict(seed=9, scale=(0.05, 1.0))
    a, _ = A.ref_boxes(np.arange(7, 27), (37, 45), **kw)
    b, _ = A.ref_boxes(np.arange(20), (37, 45), sample_base=7, **kw)
    c, _ = A.ref_boxes(np.zeros(20), (37, 45), sample_ids=np.arange(20) + 7, **kw)
    assert torch.equal(a, b) and torch.equal(a, c)
    d, _ = A.ref_boxes(np.arange(7, 27), (37, 45), seed=10, scale=(0.05, 1.0))
    assert not torch.equal(a, d)
    for p, want in ((0.0, 0), (1.0, 1)):
        f, _ = A.ref_boxes(np.arange(50), (37, 45), seed=9, flip_p=p)
        assert bool((f[:, 4] == want).all())


# --------------------------------------------------------------------- rrc_path
_PREFIX = {"cols3": "lds-cols-3", "colsn": "lds-cols-n", "rows": "lds-rows", "direct": "direct", "band4": "lds-cols-3",
           "band2": "lds-cols-3", "band1": "lds-cols-3"}


def test_crop_cases_reach_every_path():
    paths = {c.id: A.case_path(c) for c in A.CROP_CASES}
    for cid, p in paths.items():
        assert p.path == _PREFIX[cid.split("-")[0]], (cid, p)
    combos = {(p.path, p.store) for p in paths.values()}
    assert combos == {("lds-cols-3", "pair"), ("lds-cols-3", "scalar"), ("lds-cols-n", "pair"),
                      ("lds-cols-n", "scalar"), ("lds-rows", "vec4"), ("lds-rows", "scalar"), ("direct", "vec4"),
                      ("direct", "scalar")}, combos
    assert {p.band_rows for p in paths.values() if p.fits} == {16, 8, 4, 2, 1}
    assert any(not p.fits for p in paths.values())  # direct because no band height fits the budget
    for path in ("lds-cols-3", "lds-cols-n"):
        assert {p.passes for p in paths.values() if p.path == path} == {1, 2}, path
    assert any(p.fits and p.last_band_rows < p.band_rows for p in paths.values())  # a short last band
    assert {A.CROP_CASES[i].channels for i in range(len(A.CROP_CASES))} >= {1, 3, 4, 16}
    # a band whose first or last 16 B chunk straddles the image bounds: image sizes that are no multiple of 16 B
    odd = [c for c in A.CROP_CASES
           if (c.channels * c.in_hw[0] * c.in_hw[1] * torch.empty((), dtype=c.in_dtype).element_size()) % 16]
    assert odd and all(paths[c.id].path == "lds-rows" for c in odd)
    assert {c.how for c in A.CROP_CASES} == set(R.HOWS)
    assert {c.in_dtype for c in A.CROP_CASES} == {U8, BF16, F32}


def test_moat_cases_reach_every_path_and_edge():
    paths = {A.case_path(c).path for c in A.MOAT_CASES}
    assert paths == {"lds-cols-3", "lds-cols-n", "lds-rows", "direct"}
    touch, one_px, one_wide = set(), set(), set()
    for c in A.MOAT_CASES:
        (H, W), path = c.in_hw, A.case_path(c).path
        for y, x, h, w, _ in A.case_boxes(c, A.case_rows(c))[0].tolist():
            touch |= {("top", path)} if y == 0 else set()
            touch |= {("left", path)} if x == 0 else set()
            touch |= {("bottom", path)} if y + h == H else set()
            touch |= {("right", path)} if x + w == W else set()
            if h == 1 and w == 1:
                one_px.add(path)
            elif w == 1:
                one_wide.add(path)
            assert (h, w) != (H, W) or "fallback" in c.id  # poison surrounds the other crops
    assert {e for e, _ in touch} == {"top", "left", "bottom", "right"}
    assert len(one_px) >= 2 and one_wide, (one_px, one_wide)
    assert {c.in_dtype for c in A.MOAT_CASES if A.case_path(c).path.startswith("lds-cols")} == {U8, BF16, F32}


def test_exact_tier_reaches_heads_widths_and_bands():
    el = {U8: 1, BF16: 2, F32: 4}
    seen = set()
    for dt in A.EXACT_DTYPES:
        for layout in A.EXACT_LAYOUTS:
            for C in A.EXACT_CHANNELS:
                for hw in A.EXACT_HW:
                    for size in A.exact_sizes(hw):
                        p = A.rrc_path(dt, layout, C, hw, size, src_ptr=el[dt])
                        assert p.fits
                        seen.add((p.path, p.store, p.head != 0, p.last_band_rows < p.band_rows))
    # the column form off the allocation's alignment. Three channels on a 16 B pitch make the width a multiple of
    # 4 (HWC) or 16 (CHW), and so are half and twice it: odd widths of that instance are left to the crop tier
    assert {("lds-cols-3", "pair", True), ("lds-cols-n", "pair", True), ("lds-cols-n", "scalar", True)} \
        <= {s[:3] for s in seen}
    assert ("lds-rows", "vec4") in {s[:2] for s in seen} and ("lds-rows", "scalar") in {s[:2] for s in seen}
    assert any(s[3] for s in seen)  # out_h that is no multiple of the band height
    wide = [(w, A.rrc_path(w.in_dtype, w.layout, w.channels, w.in_hw, w.out_hw)) for w in A.EXACT_WIDE]
    assert all(p.path.startswith("lds-cols") for _, p in wide)
    assert {w.out_hw[1] for w, p in wide if p.passes == 2} >= {258, 512}
    assert any(p.store == "scalar" and p.path == "lds-cols-n" for _, p in wide)
    assert any(p.last_band_rows < p.band_rows for _, p in wide)
    for w, _ in wide:  # the three exact resizes only
        assert any(tuple(w.out_hw) == s for s in A.exact_sizes(w.in_hw))


def test_rrc_path_budget_and_impl():
    fits = A.rrc_path(F32, "hwc", 3, (40, 1200), (24, 48))
    assert fits.path == "direct" and not fits.fits and fits.band_rows == 16
    forced = A.rrc_path(U8, "chw", 3, (64, 64), (24, 32), impl="direct")
    assert forced.path == "direct" and forced.fits and forced.store == "vec4"
    assert A.rrc_path(F32, "chw", 3, (6, 800), (5, 40)).band_rows == 1
    assert A.rrc_path(U8, "chw", 3, (256, 320), (224, 224)).path == "lds-cols-3"  # the loaders' geometry


@pytest.mark.parametrize("in_dtype", A.EXACT_DTYPES, ids=R.name)
def test_exact_affine_survives_mean_std(in_dtype):
    for C in A.EXACT_CHANNELS:
        sc, bi, mean, std = A.affine_of(C, in_dtype, exact=True)
        assert (sc, bi) == R.exact_affine(C) and len(mean) == len(std) == C
