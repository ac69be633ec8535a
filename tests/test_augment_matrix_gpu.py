"""The fused RandomResizedCrop kernel (csrc/kernels/augment.hip) against the independent float64 references of
tests/augment_refs.py, on every dispatch path that ``augment_refs.rrc_path`` tells apart.

* Boxes: ``return_boxes=True`` equals ``ref_boxes`` on all five fields for every sample the reference does not
  flag as ambiguous; at most 2 % may be flagged (the shares measured on the CPU are beside ``BOX_CASES``).
* Exact tier: whole-image crops of small-integer pixels resized by 1, 1/2 and 2 under an exact affine are bit-exact
  (``assert_same``), for float32 and bfloat16 output.
* Random-crop tier: float32 output within the per-pixel bound derived in augment_refs; bfloat16 output equal, bit
  for bit, to the RNE bfloat16 of the float32 output of the same call.
* Moat: pixels outside each image's crop box are poison and must not reach the output.

The op allocates its output, so no guard elements surround it; the allocation the output is about to reuse is
filled with NaN first (``_dirty``) and the whole tensor is compared, which shows an element left unwritten.
"""

import numpy as np
import pytest
import torch

from ddl_amd import ops
from ddl_amd.permutation import FeistelPermutation
from tests import augment_refs as A
from tests import kernel_refs as R
from tests.kernel_refs import BF16, F32, U8

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _dirty(batch, channels, size, out_dtype):
    """Fill the block the caching allocator hands out next for this output with NaN, and release it."""
    t = torch.full((batch, channels, *size), float("nan"), dtype=out_dtype, device=_dev())
    del t


def _crop(src, rows: R.Rows, size, out_dtype, **kw):
    _dirty(len(rows), src.shape[1] if kw.get("layout", "chw") == "chw" else src.shape[-1], size, out_dtype)
    out, boxes = ops.random_resized_crop(src, size=size, out_dtype=out_dtype, return_boxes=True,
                                         **rows.kw(_dev()), **kw)
    return out, boxes.cpu()


def _assert_boxes(boxes, ref, amb, what):
    share = float(amb.double().mean())
    assert share <= A.MAX_AMBIGUOUS, f"{what}: {share:.2%} of the samples are ambiguous"
    bad = (boxes != ref).any(1) & ~amb
    if bad.any():
        i = torch.nonzero(bad).reshape(-1)[:5].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {int((~amb).sum())} unambiguous boxes differ; first at "
                             f"{i}: device {boxes[i].tolist()} reference {ref[i].tolist()}")


# ------------------------------------------------------------------------ boxes
def _draw(in_hw, n, **kw):
    """Boxes of samples 0 .. n-1 of an image size: one zero image, gathered n times, keyed by ``sample_ids``;
    2x2 outputs, so the pixel work is nil."""
    src = torch.zeros((1, 1, *in_hw), dtype=U8, device=_dev())
    idx = torch.zeros(n, dtype=torch.int64, device=_dev())
    ids = torch.arange(n, dtype=torch.int64, device=_dev())
    _, boxes = ops.random_resized_crop(src, idx, size=(2, 2), sample_ids=ids, return_boxes=True, **kw)
    return boxes.cpu()


@pytest.mark.parametrize("case", A.BOX_CASES, ids=lambda c: c.id)
def test_boxes_match_reference(case):
    """Default and wide scale ranges, both centre-crop fallbacks (8x400: ratio above ratio_max, 400x8: below
    ratio_min; every sample falls back), a square image under ratio (2, 3) where some do, and 1x1 crops."""
    boxes = _draw(case.in_hw, case.n, seed=case.seed, scale=case.scale, ratio=case.ratio)
    ref, amb = A.ref_boxes(np.arange(case.n), case.in_hw, seed=case.seed, scale=case.scale, ratio=case.ratio)
    _assert_boxes(boxes, ref, amb, case.id)


def test_box_keys():
    """The key is sample_base + source row (identity, explicit index, Feistel permutation with a base) or
    sample_base + sample_ids[i]; flip_p of 0 and 1 never / always flips."""
    n_src, n, hw, dev = 300, 200, (37, 45), _dev()
    src = torch.zeros((n_src, 1, *hw), dtype=U8, device=dev)
    kw = dict(size=(2, 2), seed=9, scale=(0.05, 1.0), return_boxes=True)
    rkw = dict(seed=9, scale=(0.05, 1.0))
    idx = torch.from_numpy(np.random.default_rng(3).integers(0, n_src, n))
    p = FeistelPermutation(n_src, seed=4, epoch=1)
    ids = torch.from_numpy(np.random.default_rng(4).integers(0, 2 ** 40, n))
    runs = {
        "identity": (dict(base=3, n_rows=n), dict(rows=np.arange(3, 3 + n))),
        "index": (dict(index=idx.to(dev)), dict(rows=idx.numpy())),
        "perm": (dict(perm=p, base=17, n_rows=n), dict(rows=p(np.arange(17, 17 + n, dtype=np.int64)))),
        "sample_ids": (dict(index=idx.to(dev), sample_ids=ids.to(dev)), dict(rows=idx.numpy(), sample_ids=ids.numpy())),
        "sample_base": (dict(base=3, n_rows=n, sample_base=1000), dict(rows=np.arange(3, 3 + n), sample_base=1000)),
        "base-and-ids": (dict(index=idx.to(dev), sample_ids=ids.to(dev), sample_base=77),
                         dict(rows=idx.numpy(), sample_ids=ids.numpy(), sample_base=77)),
    }
    got = {}
    for name, (okw, refkw) in runs.items():
        _, b = ops.random_resized_crop(src, **okw, **kw)
        got[name] = b.cpu()
        ref, amb = A.ref_boxes(refkw.pop("rows"), hw, **refkw, **rkw)
        _assert_boxes(got[name], ref, amb, name)
    # sample_base = k with row i is sample_base = 0 with sample_ids = i + k: the same key, so the same bits
    k = 1000
    shifted = torch.arange(3 + k, 3 + k + n, dtype=torch.int64, device=dev)
    _, b = ops.random_resized_crop(src, base=3, n_rows=n, sample_ids=shifted, **kw)
    assert torch.equal(b.cpu(), got["sample_base"])
    assert not torch.equal(got["identity"], got["sample_base"])
    for flip_p, want in ((0.0, 0), (1.0, 1)):
        _, b = ops.random_resized_crop(src, base=3, n_rows=n, flip_p=flip_p, **kw)
        assert bool((b[:, 4] == want).all()) and torch.equal(b[:, :4].cpu(), got["identity"][:, :4])


# ------------------------------------------------------------------- exact tier
def _run_exact(in_dtype, layout, C, in_hw, out_hw, hows, seed):
    dev = _dev()
    H, W = in_hw
    src = A.images(in_dtype, layout, C, in_hw, "ints", seed)
    sc, bi, mean, std = A.affine_of(C, in_dtype, exact=True)
    sources = {"aligned": src.to(dev), "offset": R.offset_view(src.to(dev), 1)}
    assert sources["offset"].data_ptr() % 16 != 0  # ops takes it: the column form then runs with head != 0
    whole = A.whole_image_kw(in_hw)
    for how in hows:
        rows = R.rows_of(A.N_SRC, A.BATCH, how, seed)
        boxes, amb = A.ref_boxes(rows.rows.numpy(), in_hw, seed=seed, **whole)
        assert not bool(amb.any()) and bool((boxes[:, :4] == torch.tensor([0, 0, H, W], dtype=torch.int32)).all())
        ref = A.ref_resample(src, rows.rows, boxes, out_hw, layout, F32, sc, bi)
        assert torch.equal(ref.value, ref.value.float().double())  # exactly representable: nothing was rounded
        want = {F32: ref.out, BF16: R._round(ref.value, BF16)}
        for impl in A.EXACT_IMPLS:
            for out_dtype in (F32, BF16):
                for where, s in sources.items():
                    what = f"{R.name(in_dtype)} {layout} C={C} {in_hw}->{out_hw} {how} {impl} {R.name(out_dtype)} {where}"
                    out, b = _crop(s, rows, out_hw, out_dtype, seed=seed, layout=layout, mean=mean, std=std,
                                   impl=impl, **whole)
                    assert torch.equal(b, boxes), what
                    R.assert_same(out, want[out_dtype], what)


@pytest.mark.parametrize("C", A.EXACT_CHANNELS)
@pytest.mark.parametrize("layout", A.EXACT_LAYOUTS)
@pytest.mark.parametrize("in_dtype", A.EXACT_DTYPES, ids=R.name)
def test_whole_image_resizes_are_bit_exact(in_dtype, layout, C):
    """out = in (a gather + flip + cast), in / 2 (weights 1/2) and 2 * in (weights 1/4, 3/4 and the clamp at 0), for
    every addressing mode, impl, output dtype, and a source one element off its allocation."""
    for in_hw in A.EXACT_HW:
        for out_hw in A.exact_sizes(in_hw):
            _run_exact(in_dtype, layout, C, in_hw, out_hw, R.HOWS, seed=7)


@pytest.mark.parametrize("w", A.EXACT_WIDE, ids=lambda w: f"{R.name(w.in_dtype)}-{w.layout}-c{w.channels}-{w.out_hw[1]}")
def test_wide_and_odd_widths_are_bit_exact(w):
    """Two passes of the column loop (258 leaves a partial last group of columns; 512), odd widths on a 16 B pitch
    (scalar stores), and output heights that end in a band shorter than the others."""
    _run_exact(w.in_dtype, w.layout, w.channels, w.in_hw, w.out_hw, ("perm",), seed=8)


def test_more_than_16_channels_is_rejected():
    src = torch.zeros((2, 17, 8, 8), dtype=U8, device=_dev())
    with pytest.raises(ValueError):
        ops.random_resized_crop(src, size=(4, 4))
    with pytest.raises(ValueError):
        ops.random_resized_crop(src.movedim(1, -1).contiguous(), size=(4, 4), layout="hwc", out_dtype=F32)


# ------------------------------------------------------------- random-crop tier
@pytest.mark.parametrize("kind", ["noise", "ramp"])
@pytest.mark.parametrize("case", A.CROP_CASES, ids=lambda c: c.id)
def test_random_crops_within_the_derived_bound(case, kind):
    """Compared at the *reference's* boxes. ``impl="lds"`` raises exactly where ``rrc_path`` says no band fits
    the budget; uniform noise is the worst gradient, on the smooth ramp the bound is tight enough that half a
    pixel shows (test_augment_refs.py proves both on these inputs with mutated references)."""
    dev = _dev()
    rows = A.case_rows(case)
    boxes, amb = A.case_boxes(case, rows)
    keep = ~amb
    src = A.images(case.in_dtype, case.layout, case.channels, case.in_hw, kind, case.seed)
    sc, bi, mean, std = A.affine_of(case.channels, case.in_dtype)
    ref = A.ref_resample(src, rows.rows, boxes, case.out_hw, case.layout, F32, sc, bi)
    kw = dict(seed=case.seed, scale=case.scale, ratio=case.ratio, layout=case.layout, mean=mean, std=std)
    for where, s in (("aligned", src.to(dev)), ("offset", R.offset_view(src.to(dev), 1))):
        for impl in A.EXACT_IMPLS:
            what = f"{case.id} {kind} {impl} {where}"
            if impl == "lds" and not A.case_path(case, s.data_ptr(), impl).fits:
                with pytest.raises(ValueError):
                    _crop(s, rows, case.out_hw, F32, impl=impl, **kw)
                continue
            out32, b = _crop(s, rows, case.out_hw, F32, impl=impl, **kw)
            _assert_boxes(b, boxes, amb, what)
            A.assert_resampled(out32, ref, what, keep)
            out16, b16 = _crop(s, rows, case.out_hw, BF16, impl=impl, **kw)
            assert torch.equal(b16, b), what
            A.assert_bf16_of(out16, out32, what)


# ------------------------------------------------------------------------- moat
@pytest.mark.parametrize("case", A.MOAT_CASES, ids=lambda c: c.id)
def test_no_tap_leaves_the_crop_box(case):
    """Boxes do not depend on pixel content, so the source can be built around them: NaN outside each image's box
    for float sources (the output must be finite and equal to the reference of the unpoisoned images), 255 outside
    and 0 inside for uint8 (the output must be exactly the affine of 0: the zero-weight edge tap of the column form
    may read a 255 but must not let it through)."""
    dev = _dev()
    rows = A.case_rows(case)
    ref_b, amb = A.case_boxes(case, rows)
    benign = A.images(case.in_dtype, case.layout, case.channels, case.in_hw, "noise", case.seed)
    sc, bi, mean, std = A.affine_of(case.channels, case.in_dtype)
    kw = dict(seed=case.seed, scale=case.scale, ratio=case.ratio, layout=case.layout, mean=mean, std=std)
    _, boxes = _crop(benign.to(dev), rows, case.out_hw, F32, **kw)
    _assert_boxes(boxes, ref_b, amb, case.id)

    is_u8 = case.in_dtype == U8
    chw = benign if case.layout == "chw" else benign.movedim(-1, 1)  # a view: writes go through
    if is_u8:
        poisoned = torch.full_like(benign, 255)
    else:
        poisoned = torch.full_like(benign, float("nan"))
    pview = poisoned if case.layout == "chw" else poisoned.movedim(-1, 1)
    for r, (y, x, h, w, _) in zip(rows.rows.tolist(), boxes.tolist()):
        pview[r, :, y:y + h, x:x + w] = 0 if is_u8 else chw[r, :, y:y + h, x:x + w]
    if is_u8:
        v = torch.tensor([A._f32(b) for b in bi], dtype=torch.float64).view(1, -1, 1, 1)
        want32 = R._round(v.expand(len(rows), case.channels, *case.out_hw).contiguous(), F32)
    else:
        ref = A.ref_resample(benign, rows.rows, boxes, case.out_hw, case.layout, F32, sc, bi)
    src = poisoned.to(dev)
    for impl in A.EXACT_IMPLS:
        what = f"{case.id} {impl}"
        if impl == "lds" and not A.case_path(case, src.data_ptr(), impl).fits:
            continue
        out32, b = _crop(src, rows, case.out_hw, F32, impl=impl, **kw)
        assert torch.equal(b, boxes), what
        out16, _ = _crop(src, rows, case.out_hw, BF16, impl=impl, **kw)
        if is_u8:
            R.assert_same(out32, want32, what)
        else:
            A.assert_resampled(out32, ref, what)
        A.assert_bf16_of(out16, out32, what)
