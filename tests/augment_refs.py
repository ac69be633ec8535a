"""Independent float64 references, the comparison rule and the case tables for the fused RandomResizedCrop
kernel (csrc/kernels/augment.hip, ``ops.random_resized_crop``).

Nothing here calls a project op or ``F.interpolate``: the crop boxes and the resampling are written out from the
kernel's documented meaning in numpy float64. ``tests/test_augment_refs.py`` checks the references themselves on
the CPU (against ``F.interpolate``, against deliberate mutants, and for path coverage of the tables),
``tests/test_augment_matrix_gpu.py`` runs the tables through the HIP kernels.

Crop boxes (``ref_boxes``) and ``EPS``
--------------------------------------
The device evaluates the draw in float32. With u = 2^-24 (half a float32 ulp, relative) the chain of one attempt is

* ``target = area * (smin + (smax - smin) * U)``: one subtraction, two products and one sum, <= 4u relative;
* ``aspect = expf(lr0 + (lr1 - lr0) * U)``: ``logf`` twice (<= 1 ulp = 2u of |lr| each), a difference, a product
  and a sum leave an absolute error of about 4u * |lr| <= 4.4u in the argument (|lr| <= log 3 for the box cases),
  which is the relative error of the exponential; ``expf`` itself adds <= 2u: <= 6.4u relative;
* ``target * aspect`` or ``target / aspect``: one more rounding, <= 11.4u in all; the square root halves a relative
  error and rounds once: <= 6.7u, i.e. about 3.4 float32 ulps of the pre-rounding ``w`` or ``h``. A compiler that
  contracts a product and a sum into one fused operation only removes roundings.

``EPS = 2^-18 = 64u`` is about ten times that (five times at the moat's ratio of 0.02, |lr| = 3.9: 12.5u). The products ``U * (H - h + 1)`` and the fallback quotients are one
float32 operation on exact operands (<= u), far inside the same margin. A draw whose float64 value comes within
``EPS * max(v, 1)`` of a rounding boundary at any step the device also evaluates is *ambiguous*: the device may
legitimately land on the other side. Tests drop such samples, and may drop at most ``MAX_AMBIGUOUS`` (2 %) of a case;
the share that each case of ``BOX_CASES`` flags on the CPU is recorded next to it.

Resampling (``ref_resample``) and the bound of ``assert_resampled``
-------------------------------------------------------------------
Output pixel (oy, ox) of a crop (y, x, h, w, flip) reads the crop at ``sy = max((oy + 0.5) * h / oh - 0.5, 0)`` and
``sx`` alike, from column ``ow - 1 - ox`` when flipped; ``y0 = min(floor(sy), h - 1)``, the neighbour
``min(y0 + 1, h - 1)``, weights ``sy - y0``; value ``top + (bot - top) * wy`` of the two row interpolations, then
``v * scale[c] + bias[c]``. All in float64; one rounding to float32 and the cast to the output dtype at the end.

The kernel does the same in float32. Its coordinate ``fl(fl((o + 0.5) * fl(h / oh)) - 0.5)`` has three roundings
((o + 0.5) is exact): <= 2u * (s + 0.5) from the quotient and the product, <= u * s from the difference, so
``delta(s) = 3u * (s + 1)`` bounds it (the clamp at 0 and the weight ``s - floor(s)`` are exact). The bilinear
interpolant is continuous and piecewise linear in (sy, sx), across cell borders and the clamped crop edges too, with
slopes no larger than the spread of adjacent pixels; a coordinate error below one pixel therefore moves the value by
at most ``(delta(sx) + delta(sy)) * spread``, spread = max - min of the channel over the pixels within one pixel of
the 2x2 footprint (inside the crop). Each interpolation ``a + (b - a) * t`` with |a|, |b| <= M and t in [0, 1]
rounds three times: <= 2uM (difference) + 2uM (product, t <= 1) + uM (sum) = 5uM, and passes the errors of its
operands on as a convex combination, i.e. not enlarged; two levels give 10uM, taken as ``11uM`` to cover the terms of
second order, M = largest of the four taps. The affine is one fused multiply-add: the error so far times
``|scale[c]|`` plus one rounding ``u * |result|``. The sum of these is the per-pixel bound on |out - float64 value|
for float32 output; no literal tolerance is involved. On uint8 and small-integer sources resized by 1, 1/2 or 2 with
an exact affine every intermediate is exactly representable and the comparison is ``assert_same`` (bit-exact).

bfloat16 output has no tolerance of its own: the float math is one template and only the store differs, so it must
equal, bit for bit, the round-to-nearest-even bfloat16 of the float32 output of the same call (``assert_bf16_of``).
"""

from __future__ import annotations

import collections
import functools
import math

import numpy as np
import torch

from tests import kernel_refs as R
from tests.kernel_refs import BF16, F32, U8

U = 2.0 ** -24  # half a float32 ulp, relative
EPS = 2.0 ** -18  # ambiguity margin of ref_boxes; derivation in the module docstring
MAX_AMBIGUOUS = 0.02  # cap on the share of samples a test may drop as ambiguous (the issue's condition)
DEFAULT_SCALE, DEFAULT_RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)


# ------------------------------------------------------------------- crop boxes
def mix64(z: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser on uint64 arrays (products wrap modulo 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def unit_uniform(seed: int, sample: np.ndarray, k: int) -> np.ndarray:
    """Uniform k of a sample: the top 24 bits of the hash, as an exact multiple of 2^-24 in [0, 1)."""
    inner = sample * np.uint64(0x9E3779B97F4A7C15) + np.uint64(k)
    z = mix64(np.uint64(seed & (2 ** 64 - 1)) ^ mix64(inner))
    return (z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


def _f32(v) -> float:
    return float(np.float32(v))


def _near_half(v, eps):
    return np.abs(v - np.floor(v) - 0.5) < eps * np.maximum(v, 1.0)


def _near_int(v, eps):
    return np.abs(v - np.rint(v)) < eps * np.maximum(v, 1.0)


def ref_boxes(rows, in_hw, *, seed, scale=DEFAULT_SCALE, ratio=DEFAULT_RATIO, flip_p=0.5, sample_base=0,
              sample_ids=None, eps=EPS):
    """(boxes [B, 5] int32 tensor (y, x, h, w, flip), ambiguous [B] bool tensor) of ``draw_crop``.

    The key of image i is ``sample_base + sample_ids[i]``, or ``sample_base + rows[i]`` (its source row) without
    ``sample_ids``. Ten attempts t use uniforms 2t (area), 2t + 1 (log-uniform ratio), 20 + 2t (y), 21 + 2t (x);
    the first whose rounded w, h fit the image wins; otherwise the centre crop with the image's ratio clamped
    into ``ratio``. Uniform 40 against ``flip_p`` gives the flip."""
    H, W = in_hw
    key = np.asarray(sample_ids if sample_ids is not None else rows, dtype=np.int64).reshape(-1) + np.int64(sample_base)
    sample = key.astype(np.uint64)
    n = sample.size
    smin, smax, rmin, rmax = _f32(scale[0]), _f32(scale[1]), _f32(ratio[0]), _f32(ratio[1])
    area, lr0, lr1 = float(H) * float(W), math.log(rmin), math.log(rmax)
    y, x, h, w = (np.zeros(n, dtype=np.int64) for _ in range(4))
    done, amb = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for t in range(10):
        target = area * (smin + (smax - smin) * unit_uniform(seed, sample, 2 * t))
        aspect = np.exp(lr0 + (lr1 - lr0) * unit_uniform(seed, sample, 2 * t + 1))
        wv, hv = np.sqrt(target * aspect), np.sqrt(target / aspect)
        amb |= ~done & (_near_half(wv, eps) | _near_half(hv, eps))
        wt, ht = np.rint(wv).astype(np.int64), np.rint(hv).astype(np.int64)
        ok = ~done & (wt > 0) & (wt <= W) & (ht > 0) & (ht <= H)
        yv = unit_uniform(seed, sample, 20 + 2 * t) * (H - ht + 1)
        xv = unit_uniform(seed, sample, 21 + 2 * t) * (W - wt + 1)
        amb |= ok & (_near_int(yv, eps) | _near_int(xv, eps))
        yt = np.minimum(np.floor(yv).astype(np.int64), H - ht)
        xt = np.minimum(np.floor(xv).astype(np.int64), W - wt)
        for dst, val in ((y, yt), (x, xt), (h, ht), (w, wt)):
            dst[ok] = val[ok]
        done |= ok
    fb = ~done  # centre crop, ratio clamped into [rmin, rmax]
    if fb.any():
        in_ratio = float(W) / float(H)
        fw, fh, near = W, H, False
        if in_ratio < rmin:
            fh = min(H, max(1, int(np.rint(W / rmin))))
            near = bool(_near_half(np.float64(W / rmin), eps))
        elif in_ratio > rmax:
            fw = min(W, max(1, int(np.rint(H * rmax))))
            near = bool(_near_half(np.float64(H * rmax), eps))
        near = near or min(abs(in_ratio - rmin), abs(in_ratio - rmax)) < eps * max(in_ratio, 1.0)  # branch taken
        h[fb], w[fb], y[fb], x[fb] = fh, fw, (H - fh) // 2, (W - fw) // 2
        amb |= fb & near
    flip = (unit_uniform(seed, sample, 40) < _f32(flip_p)).astype(np.int64)  # exact on both sides: never ambiguous
    boxes = torch.from_numpy(np.stack([y, x, h, w, flip], axis=1).astype(np.int32))
    return boxes, torch.from_numpy(amb)


# ------------------------------------------------------------------- resampling
Resampled = collections.namedtuple("Resampled", "value bound out")
"""``value``: float64 [B, C, oh, ow] before any rounding; ``bound``: the derived per-pixel bound on
|float32 output - value|; ``out``: ``value`` rounded to float32 and cast to the output dtype."""

MUTATIONS = ("shift_x", "shift_y", "no_clamp_x", "no_clamp_y", "no_flip", "no_half", "plane_next", "plane_prev",
             "affine_next")


def _axis(o, n_in, n_out, half=0.5):
    s = np.maximum((o + half) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    return s, i0, np.minimum(i0 + 1, n_in - 1), s - i0


def _resample(src, rows, boxes, size, layout, out_dtype, scale, bias, mutate=None) -> Resampled:
    """``mutate`` (one of ``MUTATIONS``) builds a deliberately wrong resampler; tests/test_augment_refs.py uses
    it to prove that ``assert_resampled`` rejects each of them. Mutants that read outside the crop wrap around the
    image, as a kernel reading past a row or a plane would."""
    assert mutate is None or mutate in MUTATIONS
    oh, ow = size
    x = src[torch.as_tensor(rows, dtype=torch.int64)]
    if layout == "hwc":
        x = x.movedim(-1, 1)
    imgs = x.double().numpy()
    B, C, H, W = imgs.shape
    sc = np.array([_f32(v) for v in scale], dtype=np.float64).reshape(C, 1, 1) if scale else None
    bi = np.array([_f32(v) for v in bias], dtype=np.float64).reshape(C, 1, 1) if scale else None
    if mutate == "affine_next" and scale:
        sc, bi = np.roll(sc, -1, axis=0), np.roll(bi, -1, axis=0)
    half = 0.0 if mutate == "no_half" else 0.5
    value = np.empty((B, C, oh, ow), dtype=np.float64)
    bound = np.empty_like(value)
    for i, (by, bx, bh, bw, flip) in enumerate(np.asarray(boxes).tolist()):
        img = imgs[i]
        if mutate in ("plane_next", "plane_prev"):
            img = np.roll(img, -1 if mutate == "plane_next" else 1, axis=0)
        ox = np.arange(ow)
        if flip and mutate != "no_flip":
            ox = ow - 1 - ox
        sy, ya, yb, wy = _axis(np.arange(oh), bh, oh, half)
        sx, xa, xb, wx = _axis(ox, bw, ow, half)
        if mutate == "shift_y":
            ya, yb = ya + 1, yb + 1
        if mutate == "shift_x":
            xa, xb = xa + 1, xb + 1
        if mutate == "no_clamp_y":
            yb = ya + 1
        if mutate == "no_clamp_x":
            xb = xa + 1

        def tap(yy, xx):
            return img[:, (by + yy) % H][:, :, (bx + xx) % W]  # [C, oh, ow]

        v00, v01, v10, v11 = tap(ya, xa), tap(ya, xb), tap(yb, xa), tap(yb, xb)
        wxb, wyb = wx.reshape(1, 1, ow), wy.reshape(1, oh, 1)
        top, bot = v00 + (v01 - v00) * wxb, v10 + (v11 - v10) * wxb
        v = top + (bot - top) * wyb
        # the bound (module docstring): coordinate error times the local spread, plus the interpolation roundings
        near = [tap(np.clip(ya + dy, 0, bh - 1), np.clip(xa + dx, 0, bw - 1)) for dy in (-1, 0, 1, 2)
                for dx in (-1, 0, 1, 2)]
        spread = np.maximum.reduce(near) - np.minimum.reduce(near)
        big = np.maximum.reduce([np.abs(t) for t in (v00, v01, v10, v11)])
        delta = (3 * U * (sx + 1)).reshape(1, 1, ow) + (3 * U * (sy + 1)).reshape(1, oh, 1)
        err = delta * spread + 11 * U * big
        if sc is not None:
            v = v * sc + bi
            err = np.abs(sc) * err
            err = err + U * (np.abs(v) + err)
        value[i], bound[i] = v, err
    value = torch.from_numpy(value)
    return Resampled(value, torch.from_numpy(bound), R._round(value, out_dtype))


def ref_resample(src, rows, boxes, size, layout, out_dtype, scale=None, bias=None) -> Resampled:
    """Bilinear crop-and-resize (align_corners=False) of CPU images ``src[rows]`` at ``boxes`` [B, 5], as explicit
    float64 gathers. ``scale`` / ``bias`` are the per-channel affine the kernel receives (taken at their float32
    values); empty or None: no affine."""
    return _resample(src, rows, boxes, size, layout, out_dtype, scale, bias)


def assert_resampled(out: torch.Tensor, ref: Resampled, what: str = "", keep=None) -> None:
    """float32 ``out`` within the derived per-pixel bound of the float64 reference, and finite; ``keep`` ([B] bool)
    restricts the comparison to those images."""
    assert out.dtype == F32, f"{what}: assert_resampled compares float32 output (bf16: assert_bf16_of)"
    assert tuple(out.shape) == tuple(ref.value.shape), f"{what}: shape {tuple(out.shape)} != {tuple(ref.value.shape)}"
    o = out.detach().cpu().double()
    value, bound = ref.value, ref.bound
    if keep is not None:
        keep = torch.as_tensor(keep, dtype=torch.bool)
        o, value, bound = o[keep], value[keep], bound[keep]
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite output"
    d = (o - value).abs()
    bad = d > bound
    if bad.any():
        idx = torch.nonzero(bad)[:6].tolist()
        vals = [(o[tuple(i)].item(), value[tuple(i)].item(), bound[tuple(i)].item()) for i in idx]
        worst = float((d / bound.clamp_min(1e-300))[bad].max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} pixels beyond the bound (worst {worst:.3g}x); "
                             f"first at [kept image, c, oy, ox] = {idx}; (out, ref, bound) = {vals}")


def assert_bf16_of(out16: torch.Tensor, out32: torch.Tensor, what: str = "") -> None:
    """bf16 output == RNE bf16 of the float32 output of the same call, bit for bit."""
    assert out16.dtype == BF16 and out32.dtype == F32, what
    R.assert_same(out16, out32.detach().cpu().to(BF16), what)


# --------------------------------------------------------------- dispatch mirror
RrcPath = collections.namedtuple("RrcPath", "path band_rows last_band_rows store passes fits head")


def rrc_path(in_dtype, layout, C, in_hw, out_hw, src_ptr=0, impl="auto") -> RrcPath:
    """What ``random_resized_crop`` runs for a geometry (csrc/kernels/augment.hip: ``plan_band`` and the branches of
    ``rrc_band_kernel``); a mirror of their conditions, kept here so that a change of the dispatch that leaves a
    path untested fails the coverage assertion of test_augment_refs.py.

    ``path``: ``direct`` (taps from global memory: no band height fits the 32 KiB budget, or ``impl="direct"``),
    ``lds-rows`` (row-major form over the LDS band), ``lds-cols-3`` / ``lds-cols-n`` (column form, 3 channels /
    runtime channel loop; needs a row pitch and, for CHW, a plane size that are multiples of 16 B).
    ``band_rows``: output rows per workgroup; ``last_band_rows``: those of an image's last band; ``store``: ``pair``
    or ``scalar`` (column form, by out_w % 2), ``vec4`` or ``scalar`` (otherwise, by out_w % 4); ``passes``:
    ceil(out_w / 256) column passes; ``fits``: False where ``impl="lds"`` must raise; ``head``: offset of a
    whole-row crop's first byte within its 16 B chunk on the column form (``src_ptr % 16``: images are then
    multiples of 16 B)."""
    elem = torch.empty((), dtype=in_dtype).element_size()
    (in_h, in_w), (out_h, out_w) = in_hw, out_hw
    planes, cin = (1, C) if layout == "hwc" else (C, 1)
    stride = (in_w * cin * elem + 15 + 15) // 16 * 16
    band, fits, r = 16, False, 16
    while r >= 1 and not fits:
        rows = min(-(-(r - 1) * in_h // out_h) + 3, in_h + 1)
        if planes * rows * stride <= 32 * 1024:
            band, fits = r, True
        r //= 2
    pitch, plane = in_w * cin * elem, in_h * in_w * elem
    cols = False
    if impl == "direct" or not fits:
        path, band = "direct", 16
    elif pitch % 16 == 0 and (planes == 1 or plane % 16 == 0):
        path, cols = ("lds-cols-3" if C == 3 else "lds-cols-n"), True
    else:
        path = "lds-rows"
    store = ("pair" if out_w % 2 == 0 else "scalar") if cols else ("vec4" if out_w % 4 == 0 else "scalar")
    last = out_h - (-(-out_h // band) - 1) * band
    return RrcPath(path, band, last, store, -(-out_w // 256), fits, src_ptr % 16)


# ----------------------------------------------------------------------- affines
def mean_std_for(scale, bias, in_dtype):
    """``mean`` / ``std`` that make ``ops.norm_affine`` hand the kernel exactly the float32 ``scale`` / ``bias``
    (the op takes no raw affine). Asserted here, so an inexact inversion cannot slip into a bit-exact test."""
    from ddl_amd.ops import norm_affine, pixel_max

    in_max = pixel_max(in_dtype)
    std = [1.0 / (in_max * s) for s in scale]
    mean = [-b * s for b, s in zip(bias, std)]
    sc, bi = norm_affine(len(scale), mean, std, None, None, in_max)
    assert [_f32(v) for v in sc] == [_f32(v) for v in scale] and [_f32(v) for v in bi] == [_f32(v) for v in bias]
    return mean, std


def affine_of(case_channels, in_dtype, exact=False):
    """(scale, bias, mean, std): the realistic ImageNet affine for 3 channels, ``kernel_refs.exact_affine``
    otherwise or on request."""
    if case_channels == 3 and not exact:
        sc, bi = R.realistic_affine(in_dtype)
        return sc, bi, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    sc, bi = R.exact_affine(case_channels)
    mean, std = mean_std_for(sc, bi, in_dtype)
    return sc, bi, mean, std


# ----------------------------------------------------------------------- sources
N_SRC, BATCH = 11, 8  # source images and gathered rows of every pixel case


@functools.lru_cache(maxsize=8)
def _images(dtype, layout, C, hw, kind, seed):
    H, W = hw
    g = torch.Generator().manual_seed(4000 + seed)
    if kind == "noise":  # the worst gradient
        x = (torch.randint(0, 256, (N_SRC, C, H, W), generator=g, dtype=torch.int64).double() if dtype == U8
             else torch.randn((N_SRC, C, H, W), generator=g, dtype=torch.float64) * 3)
    elif kind == "ints":  # small integers: every intermediate of an exact resize is exactly representable
        lo, hi = (0, 256) if dtype == U8 else (-64, 64)
        x = torch.randint(lo, hi, (N_SRC, C, H, W), generator=g, dtype=torch.int64).double()
    else:  # ramp: a plane per channel and image, tilted differently in each; 0 .. 250 so uint8 holds it
        yy = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1) / max(H - 1, 1)
        xx = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W) / max(W - 1, 1)
        a = ((torch.arange(C, dtype=torch.float64) + 1) / (C + 1)).view(1, C, 1, 1)
        off = (torch.arange(N_SRC, dtype=torch.float64) * 3).view(N_SRC, 1, 1, 1)
        x = 200 * (a * yy + (1 - a) * xx) + off + 10 * a
        if dtype == U8:
            x = x.floor()
    x = x.to(dtype)
    return (x.movedim(1, -1) if layout == "hwc" else x).contiguous()


def images(dtype, layout, C, hw, kind, seed=0) -> torch.Tensor:
    """[N_SRC, C, H, W] or [N_SRC, H, W, C] CPU images: ``noise``, a smooth ``ramp`` or small ``ints``."""
    return _images(dtype, layout, C, tuple(hw), kind, seed).clone()


# ------------------------------------------------------------------- case tables
BoxCase = collections.namedtuple("BoxCase", "id in_hw n scale ratio seed expect")
# ambiguous share measured on the CPU (seed 5, samples 0 .. n-1, EPS = 2^-18) beside each case; the cap is 2 %
BOX_CASES = (
    BoxCase("default-180x240", (180, 240), 2000, DEFAULT_SCALE, DEFAULT_RATIO, 5, None),  # 0.20 %
    BoxCase("default-37x45", (37, 45), 2000, DEFAULT_SCALE, DEFAULT_RATIO, 5, None),  # 0.05 %
    BoxCase("wide-scale-97x130", (97, 130), 2000, (0.05, 1.0), DEFAULT_RATIO, 5, None),  # 0.25 %
    BoxCase("fallback-wide-8x400", (8, 400), 2000, DEFAULT_SCALE, DEFAULT_RATIO, 5, "fallback"),  # 0.75 %
    BoxCase("fallback-tall-400x8", (400, 8), 2000, DEFAULT_SCALE, DEFAULT_RATIO, 5, "fallback"),  # 0.75 %
    BoxCase("square-ratio-2-3", (64, 64), 2000, (0.3, 1.0), (2.0, 3.0), 5, "some-fallback"),  # 0.55 %
    BoxCase("tiny-1x1-32x40", (32, 40), 2000, (0.0005, 0.001), DEFAULT_RATIO, 5, "1x1"),  # 0.05 %
)

Case = collections.namedtuple("Case", "id in_dtype layout channels in_hw out_hw scale ratio seed how")


def _case(id_, in_dtype, layout, channels, in_hw, out_hw, scale=DEFAULT_SCALE, ratio=DEFAULT_RATIO, seed=5,
          how="perm"):
    return Case(id_, in_dtype, layout, channels, in_hw, out_hw, scale, ratio, seed, how)


WIDE = (0.05, 1.0)
SMALL = (0.005, 0.03)  # 40 x 1200 images: crops that fit their 40 rows (larger areas all end in the centre crop)
# the random-crop tier; what each case is there for (test_augment_refs.py asserts that the list reaches every value)
CROP_CASES = (
    _case("cols3-u8-chw-pair-short-band", U8, "chw", 3, (64, 64), (24, 32), how="identity"),
    _case("cols3-u8-hwc-odd", U8, "hwc", 3, (48, 32), (20, 27), WIDE, how="index"),
    _case("cols3-u8-hwc-two-passes", U8, "hwc", 3, (16, 48), (6, 260)),
    _case("colsn-bf16-chw-c4-two-passes", BF16, "chw", 4, (40, 48), (18, 258), WIDE, how="identity"),
    _case("colsn-f32-chw-c1-odd", F32, "chw", 1, (24, 36), (24, 35), how="index"),
    _case("colsn-f32-hwc-c16-odd", F32, "hwc", 16, (12, 20), (9, 13), WIDE),
    _case("colsn-u8-hwc-c4-pair", U8, "hwc", 4, (20, 24), (12, 16), how="identity"),
    _case("rows-u8-chw-33x41-vec4", U8, "chw", 3, (33, 41), (64, 48), WIDE, how="index"),  # 4059 B images
    _case("rows-bf16-chw-97x130-band8", BF16, "chw", 3, (97, 130), (31, 29), WIDE),
    _case("rows-f32-hwc-c1-odd-image", F32, "hwc", 1, (9, 7), (11, 10), how="identity"),  # 252 B images
    _case("direct-f32-hwc-40x1200-vec4", F32, "hwc", 3, (40, 1200), (24, 48), SMALL, how="index"),
    _case("direct-f32-hwc-40x1200-scalar", F32, "hwc", 3, (40, 1200), (7, 50), SMALL),
    _case("band4-f32-chw-12x320", F32, "chw", 3, (12, 320), (10, 64), how="identity"),
    _case("band2-f32-chw-6x512", F32, "chw", 3, (6, 512), (7, 33), WIDE, how="index"),
    _case("band1-f32-chw-6x800", F32, "chw", 3, (6, 800), (5, 40)),
)

# the moat: every path, crops of one pixel and of one column, fallback crops spanning the image
MOAT_CASES = (
    _case("moat-cols3-u8-chw", U8, "chw", 3, (64, 64), (24, 32), (0.3, 1.0)),
    _case("moat-cols3-u8-hwc-odd", U8, "hwc", 3, (48, 32), (20, 27), WIDE, how="index"),
    _case("moat-colsn-u8-hwc-c4", U8, "hwc", 4, (20, 24), (12, 16), (0.3, 1.0), how="identity"),
    _case("moat-colsn-bf16-chw-c4", BF16, "chw", 4, (40, 48), (18, 258), WIDE, how="identity"),
    _case("moat-colsn-f32-chw-c1", F32, "chw", 1, (24, 36), (24, 35), (0.3, 1.0), how="index"),
    _case("moat-rows-u8-chw", U8, "chw", 3, (33, 41), (64, 48), (0.3, 1.0), how="index"),
    _case("moat-rows-bf16-chw", BF16, "chw", 3, (97, 130), (31, 29), WIDE),
    _case("moat-direct-f32-hwc", F32, "hwc", 3, (40, 1200), (7, 50), SMALL),
    _case("moat-direct-u8-hwc-wide", U8, "hwc", 16, (8, 2400), (6, 20), (0.0005, 0.003), how="identity"),
    _case("moat-1x1-u8-chw-cols", U8, "chw", 3, (32, 48), (5, 6), (0.0005, 0.001), how="identity"),
    _case("moat-1x1-f32-chw-rows", F32, "chw", 3, (32, 41), (4, 7), (0.0005, 0.001)),
    _case("moat-1-wide-u8-hwc-cols", U8, "hwc", 4, (32, 40), (9, 4), (0.008, 0.012), (0.02, 0.05), how="index"),
    _case("moat-1-wide-bf16-chw-cols", BF16, "chw", 3, (32, 40), (8, 3), (0.008, 0.012), (0.02, 0.05)),
    _case("moat-fallback-u8-chw-8x400", U8, "chw", 3, (8, 400), (6, 10), how="identity"),
    _case("moat-fallback-f32-hwc-400x8", F32, "hwc", 3, (400, 8), (10, 6), how="index"),
)


def case_rows(case: Case) -> R.Rows:
    return R.rows_of(N_SRC, BATCH, case.how, case.seed)


def case_boxes(case: Case, rows: R.Rows, flip_p=0.5):
    return ref_boxes(rows.rows.numpy(), case.in_hw, seed=case.seed, scale=case.scale, ratio=case.ratio,
                     flip_p=flip_p)


def case_path(case: Case, src_ptr=0, impl="auto") -> RrcPath:
    return rrc_path(case.in_dtype, case.layout, case.channels, case.in_hw, case.out_hw, src_ptr, impl)


# the exact tier: whole-image crops resized by 1, 1/2 and 2
EXACT_DTYPES, EXACT_LAYOUTS, EXACT_CHANNELS = (U8, BF16, F32), ("chw", "hwc"), (1, 3, 4, 16)
EXACT_HW = ((12, 32), (10, 18))  # 32-wide rows: 16 B pitch for every dtype (column form); 18-wide: mostly row-major
EXACT_IMPLS = ("auto", "lds", "direct")


def exact_sizes(in_hw):
    """out = in (weights 0), in / 2 (weights 1/2), 2 * in (weights 1/4 and 3/4, the coordinate clamp at 0)."""
    H, W = in_hw
    return ((H, W), (H // 2, W // 2), (2 * H, 2 * W))


ExactWide = collections.namedtuple("ExactWide", "in_dtype layout channels in_hw out_hw")
# two column passes (258 leaves a partial last group), odd widths on a 16 B pitch, bands of 8 output rows after 16
EXACT_WIDE = (
    ExactWide(F32, "hwc", 4, (6, 258), (6, 258)),
    ExactWide(U8, "hwc", 16, (5, 129), (10, 258)),
    ExactWide(BF16, "hwc", 4, (4, 258), (2, 129)),
    ExactWide(U8, "chw", 3, (6, 256), (12, 512)),
    ExactWide(F32, "chw", 3, (4, 512), (4, 512)),
    ExactWide(BF16, "chw", 1, (8, 1024), (4, 512)),
    ExactWide(U8, "hwc", 16, (9, 35), (9, 35)),
    ExactWide(F32, "chw", 3, (24, 36), (24, 36)),
    ExactWide(U8, "chw", 3, (12, 64), (24, 128)),
)


def whole_image_kw(in_hw) -> dict:
    """Crop parameters that force the crop to the whole image: target area = image area, ratio = W / H."""
    H, W = in_hw
    return dict(scale=(1.0, 1.0), ratio=(W / H, W / H))
