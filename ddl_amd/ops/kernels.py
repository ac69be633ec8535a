"""Python front-end of the hand-written gfx950 kernels (csrc/kernels/*.hip).

Every op dispatches to the HIP kernel when its tensors live on the GPU and to
a plain-PyTorch reference (``ref_*``) when they live on the CPU. There is no
silent fallback on GPU: if the extension is missing on a GPU host the call
raises ``NativeExtensionError`` (see ``ddl_amd._native``). Tests compare each
kernel against its ``ref_*`` (an fp32 PyTorch reference of the same op).

Row-indexing convention shared by the gather-style ops (``RowIndex`` in
csrc/kernels/common.h): output row ``r`` reads source row
  * ``index[r]``                      if ``index`` is given,
  * ``perm(base + r)``                if ``perm`` (a FeistelPermutation) is given,
  * ``base + r``                      otherwise.
"""

from __future__ import annotations

import dataclasses
import functools
import math
from typing import Sequence

import numpy as np
import torch

from .. import _native
from ..permutation import FeistelPermutation, _mix64
from . import _dtypes


@dataclasses.dataclass
class HostRows:
    """Rows living in pinned, device-mapped host memory (zero-copy source).

    ``cpu`` is a CPU tensor view of the memory ([N, *row_shape]); ``device_ptr``
    is the address the GPU uses for it (``hipHostGetDevicePointer``).
    """

    cpu: torch.Tensor
    device_ptr: int

    @property
    def shape(self):
        return self.cpu.shape

    @property
    def dtype(self):
        return self.cpu.dtype

    @property
    def device(self):
        return torch.device("cuda", torch.cuda.current_device())

    def dim(self) -> int:
        return self.cpu.dim()


def _stream_handle(stream) -> int:
    if stream is None:
        # == torch.cuda.current_stream().cuda_stream, without building a Stream object (per-launch host cost)
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


def _stream_pair(stream, dev) -> tuple:
    """(the raw handle the launchers take, what ``torch.cuda.stream`` takes for the allocations in front of them:
    a raw handle as a torch stream, None for the current stream)."""
    handle = _stream_handle(stream)
    if isinstance(stream, int):
        stream = torch.cuda.ExternalStream(stream, device=dev)
    return handle, stream


def _is_gpu(t) -> bool:
    return isinstance(t, HostRows) or (isinstance(t, torch.Tensor) and t.is_cuda)


def _same_device(out: torch.Tensor, src) -> bool:
    """``out`` can take a kernel's result for ``src``: on the source tensor's GPU (any GPU for host-mapped rows)."""
    return out.is_cuda and (isinstance(src, HostRows) or out.device == src.device)


def _src_addr(src) -> int:
    return src.device_ptr if isinstance(src, HostRows) else src.data_ptr()


def row_selector(index: torch.Tensor | None = None, perm: FeistelPermutation | None = None, base: int = 0) -> dict:
    """The ``RowIndex`` arguments of the native launchers: the rows of a device ``index``, of ``perm`` from
    position ``base`` on, or ``base, base + 1, ...``."""
    if index is not None and perm is not None:
        raise ValueError("give either index or perm, not both")
    if index is not None:
        if index.dtype != torch.int64:
            raise TypeError("index must be int64")
        if not index.is_cuda:
            raise ValueError("index must live on the GPU for a GPU gather")
        if not index.is_contiguous():
            raise ValueError("index must be contiguous")
        return dict(mode=1, idx=index.data_ptr(), base=0, keys=[0] * 6, n_domain=1, half_bits=1)
    if perm is not None:
        return dict(mode=2, idx=0, base=int(base), **perm.device_args())
    return dict(mode=0, idx=0, base=int(base), keys=[0] * 6, n_domain=1, half_bits=1)


_index_kw = row_selector

def _ref_rows(n_src: int, n_rows: int, index, perm, base) -> torch.Tensor:
    if index is not None:
        return index.to("cpu", torch.int64)
    pos = np.arange(base, base + n_rows, dtype=np.int64)
    if perm is not None:
        return torch.from_numpy(perm(pos))
    if pos.size and pos.max() >= n_src:
        raise IndexError("identity rows out of range")
    return torch.from_numpy(pos)


def _affine_lists(scale, bias) -> tuple[list[float], list[float]]:
    if scale is None and bias is None:
        return [], []
    if scale is None:
        scale = [1.0] * len(bias)
    if bias is None:
        bias = [0.0] * len(scale)
    scale, bias = [float(s) for s in scale], [float(b) for b in bias]
    if len(scale) != len(bias) or not 1 <= len(scale) <= 16:
        raise ValueError("scale/bias: 1..16 channels of equal length")
    return scale, bias


def _check_rows(src, index, perm, base, n_rows) -> int:
    n_src = src.shape[0]
    if n_rows is None:
        if index is not None:
            n_rows = index.numel()
        elif perm is not None:
            n_rows = perm.n - base
        else:
            n_rows = n_src - base
    if n_rows < 0:
        raise ValueError("negative row count")
    if perm is not None and (base < 0 or base + n_rows > perm.n):
        raise IndexError("perm positions out of range")
    if perm is not None and perm.n > n_src:
        raise IndexError("permutation domain larger than the source")
    if index is None and perm is None and base + n_rows > n_src:
        raise IndexError("identity rows out of range")
    return int(n_rows)


# --------------------------------------------------------------------- gather
def ref_gather_rows(src, index=None, perm=None, base=0, n_rows=None, out_dtype=None, scale=None, bias=None,
                    plane=None) -> torch.Tensor:
    x = src.cpu if isinstance(src, HostRows) else src
    n_rows = _check_rows(x, index, perm, base, n_rows)
    rows = x.index_select(0, _ref_rows(x.shape[0], n_rows, index, perm, base).to(x.device))
    out_dtype = out_dtype or x.dtype
    sc, bi = _affine_lists(scale, bias)
    if sc:
        flat = rows.reshape(n_rows, -1).double()
        ch = (torch.arange(flat.shape[1], device=flat.device) // int(plane)) % len(sc)
        s = torch.tensor(sc, dtype=torch.float64, device=flat.device)[ch]
        b = torch.tensor(bi, dtype=torch.float64, device=flat.device)[ch]
        rows = (flat * s + b).float().reshape(rows.shape)
    elif out_dtype != x.dtype:
        rows = rows.float()
    return rows.to(out_dtype)


def gather_rows(src, index: torch.Tensor | None = None, *, perm: FeistelPermutation | None = None, base: int = 0,
                n_rows: int | None = None, out: torch.Tensor | None = None, out_dtype=None, scale=None, bias=None,
                plane: int | None = None, stream=None, max_blocks: int = 0) -> torch.Tensor:
    """out[r] = cast(affine(src[row(r)])): fused permute + cast + per-channel normalise.

    ``max_blocks`` > 0 caps the grid (the kernel grid-strides over row tiles):
    a zero-copy gather out of pinned host memory is PCIe-latency-bound and
    saturates the link with a few dozen workgroups, leaving the other CUs to
    the training step.
    """
    if out_dtype is not None:
        out_dtype = _dtypes.to_torch_dtype(out_dtype)
    else:
        out_dtype = out.dtype if out is not None else src.dtype
    if not _is_gpu(src):
        res = ref_gather_rows(src, index, perm, base, n_rows, out_dtype, scale, bias, plane)
        if out is not None:
            out.copy_(res)
            return out
        return res
    n_rows = _check_rows(src, index, perm, base, n_rows)
    row_shape = tuple(src.shape[1:])
    row_elems = int(math.prod(row_shape)) if row_shape else 1
    if isinstance(src, torch.Tensor) and not src.is_contiguous():
        raise ValueError("gather_rows: source must be contiguous")
    if out is None:
        out = torch.empty((n_rows,) + row_shape, dtype=out_dtype, device=src.device)
    elif (not out.is_contiguous() or out.dtype != out_dtype or out.numel() != n_rows * row_elems
          or not _same_device(out, src)):
        raise ValueError("gather_rows: bad out tensor")
    sc, bi = _affine_lists(scale, bias)
    if sc and plane is None:
        raise ValueError("plane (elements per channel) is required with scale/bias")
    if sc and (out_dtype in (torch.uint8, torch.int32, torch.int64)):
        raise TypeError("normalisation needs a floating output dtype")
    if out_dtype != src.dtype and out_dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"cannot cast {src.dtype} -> {out_dtype} in the gather")
    _native.hip().gather_rows(
        dst=out.data_ptr(), out_dt=_dtypes.code(out_dtype), src=_src_addr(src), in_dt=_dtypes.code(src.dtype),
        n_rows=n_rows, row_elems=row_elems, scale=sc, bias=bi, plane=int(plane or 0), scatter=False,
        stream=_stream_handle(stream), max_blocks=int(max_blocks), host_src=isinstance(src, HostRows),
        **_index_kw(index, perm, base))
    return out


def scatter_rows(dst: torch.Tensor, src: torch.Tensor, index: torch.Tensor, *, stream=None,
                 max_blocks: int = 0) -> torch.Tensor:
    """dst[index[r]] = src[r] (same dtype). Used to put exchanged rows back. ``max_blocks`` > 0 caps the
    grid, as for ``gather_rows``."""
    if dst.dtype != src.dtype or dst.shape[1:] != src.shape[1:]:
        raise ValueError("scatter_rows: dst/src row mismatch")
    if index.numel() != src.shape[0]:
        raise ValueError("scatter_rows: one index per source row")
    if not dst.is_cuda:
        dst.index_copy_(0, index.to(torch.int64), src)
        return dst
    if src.device != dst.device or not dst.is_contiguous() or not src.is_contiguous():
        raise ValueError("scatter_rows: dst and src must be contiguous tensors on one device")
    row_elems =int(math.prod(src.shape[1:])) if src.dim() > 1 else 1
    _native.hip().gather_rows(
        dst=dst.data_ptr(), out_dt=_dtypes.code(dst.dtype), src=src.data_ptr(), in_dt=_dtypes.code(src.dtype),
        n_rows=src.shape[0], row_elems=row_elems, scale=[], bias=[], plane=0, scatter=True,
        stream=_stream_handle(stream), max_blocks=int(max_blocks), **_index_kw(index, None, 0))
    return dst


def feistel_indices(perm: FeistelPermutation, base: int, count: int, device=None, stream=None) -> torch.Tensor:
    """Materialise perm(base .. base+count-1) (int64) on ``device``."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    if base < 0 or base + count > perm.n:
        raise IndexError("positions out of range")
    if device.type != "cuda":
        return torch.from_numpy(perm(np.arange(base, base + count, dtype=np.int64)))
    out = torch.empty(count, dtype=torch.int64, device=device)
    _native.hip().feistel_indices(out=out.data_ptr(), count=count, base=base, stream=_stream_handle(stream),
                                  **perm.device_args())
    return out


def cast(x: torch.Tensor, dtype, *, scale=None, bias=None, plane=None, stream=None) -> torch.Tensor:
    """Vectorised dtype cast (RNE to bf16) with optional per-channel affine."""
    dtype = _dtypes.to_torch_dtype(dtype)
    rows = x.reshape(x.shape[0], -1) if x.dim() > 1 else x.reshape(1, -1)
    out = gather_rows(rows, out_dtype=dtype, scale=scale, bias=bias, plane=plane, stream=stream)
    return out.reshape(x.shape)


# -------------------------------------------------------------- ragged gather
def _ragged_args(src, src_offsets, idx) -> tuple[torch.Tensor, np.ndarray, np.ndarray]:
    """Checked (flat source tensor, src_start [n], dst_offsets [n + 1]) of a ragged gather."""
    flat = (src.cpu if isinstance(src, HostRows) else src).reshape(-1)
    if flat.element_size() not in (2, 4):
        raise TypeError("gather_ragged: 2- or 4-byte elements")
    offs = np.ascontiguousarray(src_offsets.numpy() if isinstance(src_offsets, torch.Tensor) else src_offsets,
                                dtype=np.int64).reshape(-1)
    idx = np.ascontiguousarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64).reshape(-1)
    if offs.size < 1 or (idx.size and (idx.min() < 0 or idx.max() >= offs.size - 1)):
        raise IndexError("gather_ragged: sequence index out of range")
    start, lens = offs[idx], offs[idx + 1] - offs[idx]
    if idx.size and (lens.min() < 0 or start.min() < 0 or (start + lens).max() > flat.numel()):
        raise ValueError("gather_ragged: source offsets decrease or run past the source")
    return flat, start, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def ref_gather_ragged(src, src_offsets, idx) -> tuple[torch.Tensor, torch.Tensor]:
    """(tokens, offsets): sequences ``idx`` of the flat ``src`` (sequence i = src[src_offsets[i]:src_offsets[i+1]])
    back to back, and their int64 running offsets [n + 1]."""
    flat, start, dofs = _ragged_args(src, src_offsets, idx)
    flat = flat.cpu()
    parts = [flat[s:s + n] for s, n in zip(start.tolist(), np.diff(dofs).tolist())]
    return (torch.cat(parts) if parts else flat[:0].clone()), torch.from_numpy(dofs)


def gather_ragged(src, src_offsets, idx, *, out: torch.Tensor | None = None, max_blocks: int = 0,
                  stream=None) -> tuple[torch.Tensor, torch.Tensor]:
    """Ragged gather on the device: ``src`` is a flat device tensor or ``HostRows`` (pinned, device-mapped host
    memory: every token crosses PCIe once, in 16-byte aligned loads); ``src_offsets`` and ``idx`` live on the
    host. Returns (tokens [sum of lengths] in ``out`` if given, offsets [n + 1] int64), both on the device.
    ``max_blocks`` > 0 caps the grid as for ``gather_rows``."""
    if not _is_gpu(src):
        tokens, dofs = ref_gather_ragged(src, src_offsets, idx)
        if out is not None:
            out.reshape(-1)[:tokens.numel()].copy_(tokens)
            return out.reshape(-1)[:tokens.numel()], dofs
        return tokens, dofs
    flat, start, dofs = _ragged_args(src, src_offsets, idx)
    if isinstance(src, torch.Tensor) and not src.is_contiguous():
        raise ValueError("gather_ragged: source must be contiguous")
    n, total, eb = int(start.size), int(dofs[-1]), flat.element_size()
    # one descriptor: src_start [n] i64, dst_offsets [n + 1] i64, tile_start [n + 1] i32
    words = np.zeros(2 * n + 1 + (n + 2) // 2, dtype=np.int64)
    words[:n], words[n:2 * n + 1] = start, dofs
    hip, addr = _native.hip(), _src_addr(src)
    n_tiles = hip.ragged_tile_plan(addr, words.ctypes.data, words[n:].ctypes.data, n, eb,
                                   words[2 * n + 1:].ctypes.data)
    dev = src.device
    if out is None:
        out = torch.empty(total, dtype=flat.dtype, device=dev)
    elif not out.is_cuda or not out.is_contiguous() or out.dtype != flat.dtype or out.numel() < total:
        raise ValueError("gather_ragged: bad out tensor")
    desc, handle, _ = _upload_words(words, dev, stream)
    base = desc.data_ptr()
    hip.gather_ragged(dst=out.data_ptr(), src=addr, src_start=base, dst_offsets=base + 8 * n,
                      tile_start=base + 8 * (2 * n + 1), n=n, n_tiles=n_tiles, elem_bytes=eb,
                      max_blocks=int(max_blocks), stream=handle)
    return out.reshape(-1)[:total], desc[n:2 * n + 1]


# -------------------------------------------------------------------- collate
def ref_collate_hwc_to_chw(src, index=None, perm=None, base=0, n_rows=None, out_dtype=torch.bfloat16, mean=None,
                           std=None, scale=None, bias=None) -> torch.Tensor:
    x = src.cpu if isinstance(src, HostRows) else src
    n_rows = _check_rows(x, index, perm, base, n_rows)
    rows = x.index_select(0, _ref_rows(x.shape[0], n_rows, index, perm, base).to(x.device))
    c = rows.shape[-1]
    sc, bi = norm_affine(c, mean, std, scale, bias, pixel_max(x.dtype))
    y = rows.double().movedim(-1, 1)  # [B, C, H, W]
    if sc:
        s = torch.tensor(sc, dtype=torch.float64, device=y.device).view(1, c, *([1] * (y.dim() - 2)))
        b = torch.tensor(bi, dtype=torch.float64, device=y.device).view(1, c, *([1] * (y.dim() - 2)))
        y = y * s + b
    return y.float().to(out_dtype).contiguous()


def pixel_max(dtype) -> float:
    """Value range the mean/std convention refers to: uint8 pixels are read as x/255
    (torchvision convention on [0, 1] images); every other dtype as raw values."""
    return 255.0 if _dtypes.to_torch_dtype(dtype) == torch.uint8 else 1.0


def norm_affine(c, mean=None, std=None, scale=None, bias=None, in_max: float = 255.0):
    """(x/in_max - mean)/std  ==  x*scale + bias  with scale=1/(in_max*std), bias=-mean/std.

    ``in_max`` is ``pixel_max(source dtype)``: 255 for uint8 sources, 1 otherwise.
    """
    if mean is not None or std is not None:
        mean = list(mean) if mean is not None else [0.0] * c
        std = list(std) if std is not None else [1.0] * c
        if len(mean) != c or len(std) != c:
            raise ValueError("mean/std must have one entry per channel")
        return [1.0 / (in_max * s) for s in std], [-m / s for m, s in zip(mean, std)]
    return _affine_lists(scale, bias)


def collate_hwc_to_chw(src, index: torch.Tensor | None = None, *, perm: FeistelPermutation | None = None,
                       base: int = 0, n_rows: int | None = None, out_dtype=torch.bfloat16, mean=None, std=None,
                       scale=None, bias=None, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """[N, H, W, C] (u8/f32/bf16, HWC) rows -> [B, C, H, W] normalised bf16/f32 (LDS-staged de-interleave).

    ``mean``/``std`` follow the torchvision convention on [0, 1] pixels for uint8
    sources (``(x/255 - mean)/std``) and apply to raw values for float sources;
    alternatively pass a raw ``scale``/``bias``.
    """
    out_dtype = _dtypes.to_torch_dtype(out_dtype)
    if src.dim() < 3:
        raise ValueError("collate_hwc_to_chw expects [N, ..., C]")
    c = src.shape[-1]
    if not _is_gpu(src):
        res = ref_collate_hwc_to_chw(src, index, perm, base, n_rows, out_dtype, mean, std, scale, bias)
        if out is not None:
            out.copy_(res)
            return out
        return res
    n_rows = _check_rows(src, index, perm, base, n_rows)
    spatial = tuple(src.shape[1:-1])
    pixels = int(math.prod(spatial))
    sc, bi = norm_affine(c, mean, std, scale, bias, pixel_max(src.dtype))
    if isinstance(src, torch.Tensor) and not src.is_contiguous():
        raise ValueError("collate_hwc_to_chw: source must be contiguous")
    if out is None:
        out = torch.empty((n_rows, c) + spatial, dtype=out_dtype, device=src.device)
    elif (not out.is_contiguous() or out.dtype != out_dtype or out.numel() != n_rows * c * pixels
          or not _same_device(out, src)):
        raise ValueError(f"collate_hwc_to_chw: out must be a contiguous {out_dtype} tensor of "
                         f"{n_rows * c * pixels} elements on {src.device}")
    try:
        _native.hip().collate_hwc_to_chw(
            dst=out.data_ptr(), out_dt=_dtypes.code(out_dtype), src=_src_addr(src), in_dt=_dtypes.code(src.dtype),
            batch=n_rows, pixels=pixels, channels=c, scale=sc, bias=bi, stream=_stream_handle(stream),
            **_index_kw(index, perm, base))
    except ValueError as e:
        if "(code -5)" not in str(e):
            raise
        # the kernel stages whole pixels in LDS: 8 of them must fit a workgroup's share
        raise ValueError(f"collate_hwc_to_chw: {c} channels of {src.dtype} do not fit the LDS tile") from e
    return out


# ---------------------------------------------------------------- augment
def ref_random_resized_crop(src, boxes, size, layout: str = "chw", index=None, perm=None, base=0, n_rows=None,
                            out_dtype=torch.bfloat16, mean=None, std=None) -> torch.Tensor:
    """Torch reference of ``random_resized_crop`` for given crop boxes [B, 5] (y, x, h, w, flip)."""
    import torch.nn.functional as F

    x = src.cpu if isinstance(src, HostRows) else src
    n_rows = _check_rows(x, index, perm, base, n_rows)
    rows = x.index_select(0, _ref_rows(x.shape[0], n_rows, index, perm, base).to(x.device)).cpu()
    if layout == "hwc":
        rows = rows.movedim(-1, 1)
    imgs = rows.float()
    c = imgs.shape[1]
    sc, bi = norm_affine(c, mean, std, None, None, pixel_max(x.dtype))
    oh, ow = size
    out = torch.empty((n_rows, c, oh, ow), dtype=torch.float32)
    for i, (y0, x0, h, w, flip) in enumerate(boxes.tolist()):
        crop = imgs[i:i + 1, :, y0:y0 + h, x0:x0 + w]
        r = F.interpolate(crop, size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)[0]
        if flip:
            r = r.flip(-1)
        if sc:
            r = r * torch.tensor(sc).view(c, 1, 1) + torch.tensor(bi).view(c, 1, 1)
        out[i] = r
    return out.to(out_dtype)


def random_resized_crop(src, index: torch.Tensor | None = None, *, perm: FeistelPermutation | None = None,
                        base: int = 0, n_rows: int | None = None, size=(224, 224), scale=(0.08, 1.0),
                        ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p: float = 0.5, seed: int = 0, sample_base: int = 0,
                        layout: str = "chw", out_dtype=torch.bfloat16, mean=None, std=None,
                        return_boxes: bool = False, impl: str = "auto", stream=None,
                        sample_ids: torch.Tensor | None = None):
    """Gathered images -> RandomResizedCrop + horizontal flip + normalise + cast, one gfx950 kernel.

    ``src`` rows are [C, H, W] (``layout="chw"``) or [H, W, C] (``"hwc"``),
    uint8 / bf16 / f32. Crop boxes follow torchvision's RandomResizedCrop
    (``scale``, ``ratio``) and are drawn on the device from
    hash(``seed``, ``sample_base`` + source row): the same sample gets the same
    crop under the same seed whichever rank or batch it lands in.
    Returns [B, C, size[0], size[1]] (and the [B, 5] int32 boxes y, x, h, w,
    flip with ``return_boxes``). ``impl``: ``"auto"`` stages each band of
    output rows' source pixels in LDS when the band fits the kernel's LDS
    budget, ``"lds"`` requires that (ValueError otherwise), ``"direct"`` reads
    every tap from global memory; all three give identical results.
    ``sample_ids`` (int64 [B] on the device) replaces the source row in the crop
    key: rows gathered out of an exchange buffer keep the crop of their global
    sample id.
    """
    paths = {"auto": 0, "lds": 1, "direct": 2}
    if impl not in paths:
        raise ValueError(f"impl must be one of {sorted(paths)}")
    out_dtype = _dtypes.to_torch_dtype(out_dtype)
    if layout not in ("chw", "hwc") or src.dim() != 4:
        raise ValueError("random_resized_crop expects [N, C, H, W] (chw) or [N, H, W, C] (hwc) rows")
    if not _is_gpu(src):
        raise RuntimeError("random_resized_crop runs on the GPU (crop boxes are drawn on the device)")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("random_resized_crop writes bf16 or f32")
    n_rows = _check_rows(src, index, perm, base, n_rows)
    if layout == "hwc":
        h, w, c = src.shape[1:]
    else:
        c, h, w = src.shape[1:]
    oh, ow = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    sc, bi = norm_affine(c, mean, std, None, None, pixel_max(src.dtype))
    dev = src.device if isinstance(src, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((n_rows, c, oh, ow), dtype=out_dtype, device=dev)
    boxes = torch.empty((n_rows, 5), dtype=torch.int32, device=dev)  # drawn by a per-image pre-pass
    ids_ptr = 0
    if sample_ids is not None:
        if sample_ids.dtype != torch.int64 or sample_ids.device != dev or sample_ids.numel() != n_rows \
                or not sample_ids.is_contiguous():
            raise ValueError("sample_ids must be a contiguous int64 [n_rows] tensor on the source's device")
        ids_ptr = sample_ids.data_ptr()
    _native.hip().random_resized_crop(
        dst=out.data_ptr(), out_dt=_dtypes.code(out_dtype), src=_src_addr(src), in_dt=_dtypes.code(src.dtype),
        batch=n_rows, hwc=layout == "hwc", in_h=int(h), in_w=int(w), channels=int(c), out_h=oh, out_w=ow,
        seed=int(seed) & ((1 << 64) - 1), sample_base=int(sample_base), scale_min=float(scale[0]),
        scale_max=float(scale[1]), ratio_min=float(ratio[0]), ratio_max=float(ratio[1]), flip_p=float(flip_p),
        scale=sc, bias=bi, boxes_out=boxes.data_ptr(), path=paths[impl], stream=_stream_handle(stream),
        sample_ids=ids_ptr, **_index_kw(index, perm, base))
    return (out, boxes) if return_boxes else out


def ref_split_columns(src, splits, index=None, perm=None, base=0, n_rows=None, out_dtype=None):
    x = src.cpu if isinstance(src, HostRows) else src
    n_rows = _check_rows(x, index, perm, base, n_rows)
    rows = x.index_select(0, _ref_rows(x.shape[0], n_rows, index, perm, base).to(x.device))
    out_dtype = out_dtype or x.dtype
    if out_dtype == x.dtype:
        return tuple(p.contiguous() for p in torch.split(rows, list(splits), dim=1))
    return tuple(p.float().to(out_dtype).contiguous() for p in torch.split(rows, list(splits), dim=1))


def split_columns(src, splits: Sequence[int], index: torch.Tensor | None = None, *,
                  perm: FeistelPermutation | None = None, base: int = 0, n_rows: int | None = None, out_dtype=None,
                  stream=None) -> tuple[torch.Tensor, ...]:
    """[N, nValues] rows -> tuple of contiguous [B, w_k] column groups (fused gather + cast)."""
    out_dtype = _dtypes.to_torch_dtype(out_dtype) if out_dtype is not None else src.dtype
    if src.dim() != 2:
        raise ValueError("split_columns expects [N, nValues]")
    if sum(splits) != src.shape[1]:
        raise ValueError("splits must sum to nValues")
    if not _is_gpu(src):
        return ref_split_columns(src, splits, index, perm, base, n_rows, out_dtype)
    if out_dtype != src.dtype and out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("split_columns casts to bf16 or f32 only (same-dtype splits are raw copies)")
    n_rows = _check_rows(src, index, perm, base, n_rows)
    # one allocation, k contiguous [n_rows, w] views (a caching-allocator call costs ~2.5 us of host time)
    buf = torch.empty(n_rows * sum(splits), dtype=out_dtype, device=src.device)
    outs, off = [], 0
    for w in splits:
        outs.append(buf[off:off + n_rows * w].view(n_rows, w))
        off += n_rows * w
    outs = tuple(outs)
    _native.hip().split_columns(
        dsts=[o.data_ptr() for o in outs], widths=[int(w) for w in splits], out_dt=_dtypes.code(out_dtype),
        src=_src_addr(src), in_dt=_dtypes.code(src.dtype), n_rows=n_rows, n_values=src.shape[1],
        stream=_stream_handle(stream), **_index_kw(index, perm, base))
    return outs


def ref_pack_columns(groups, index=None, perm=None, base=0, n_rows=None, out_dtype=None):
    g0 = groups[0]
    n_rows = _check_rows(g0, index, perm, base, n_rows)
    rows = _ref_rows(g0.shape[0], n_rows, index, perm, base).to(g0.device)
    out_dtype = out_dtype or g0.dtype
    cat = torch.cat([g.index_select(0, rows) for g in groups], dim=1)
    return cat if out_dtype == g0.dtype else cat.float().to(out_dtype)


def pack_columns(groups: Sequence[torch.Tensor], index: torch.Tensor | None = None, *,
                 perm: FeistelPermutation | None = None, base: int = 0, n_rows: int | None = None, out_dtype=None,
                 out: torch.Tensor | None = None, host_threads: int = 4, stream=None) -> torch.Tensor:
    """k [N, w_g] column groups -> one [B, sum w_g] row block.

    The reference fills each producer window by concatenating the harness's
    column groups on the host (tests/run_ddl.py:156-159). On the host this runs
    on the native thread pool (row-blocked memcpy, GIL released); on the GPU it
    is one gfx950 kernel fused with the row gather (index / Feistel perm) and
    the dtype cast -- the inverse of ``split_columns``.
    """
    groups = list(groups)
    if not 1 <= len(groups) <= 8:
        raise ValueError("pack_columns takes 1..8 groups")
    g0 = groups[0]
    for g in groups:
        if g.dim() != 2 or g.shape[0] != g0.shape[0] or g.dtype != g0.dtype or g.device != g0.device:
            raise ValueError("groups must be 2-D with equal row counts, dtype and device")
    widths = [int(g.shape[1]) for g in groups]
    n_values = sum(widths)
    out_dtype = _dtypes.to_torch_dtype(out_dtype) if out_dtype is not None else (
        out.dtype if out is not None else g0.dtype)
    n_rows = _check_rows(g0, index, perm, base, n_rows)
    if out is None:
        out = torch.empty((n_rows, n_values), dtype=out_dtype, device=g0.device)
    if tuple(out.shape) != (n_rows, n_values) or out.dtype != out_dtype or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {(n_rows, n_values)} {out_dtype} tensor")
    groups = [g.contiguous() for g in groups]
    if not g0.is_cuda:
        if index is None and perm is None and out_dtype == g0.dtype:
            esz = g0.element_size()
            _native.runtime().pack_columns(out.data_ptr(), [g.data_ptr() + base * w * esz
                                                            for g, w in zip(groups, widths)],
                                           widths, esz, n_rows, host_threads)
            return out
        out.copy_(ref_pack_columns(groups, index, perm, base, n_rows, out_dtype))
        return out
    if out_dtype != g0.dtype and out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("pack_columns casts to bf16 or f32 only (same-dtype packs are raw copies)")
    if out.device != g0.device:
        raise ValueError("out must be on the groups' device")
    _native.hip().pack_columns(
        srcs=[g.data_ptr() for g in groups], widths=widths, in_dt=_dtypes.code(g0.dtype), dst=out.data_ptr(),
        out_dt=_dtypes.code(out_dtype), n_rows=n_rows, n_values=n_values, stream=_stream_handle(stream),
        **_index_kw(index, perm, base))
    return out


# --------------------------------------------------------------------- tokens
_TOK16 = (torch.int16, torch.uint16)


def widen_tokens(tokens: torch.Tensor) -> torch.Tensor:
    """int32 view of a token tensor: int32 as is; 2-byte tokens (uint16 ids on the wire, int16-typed views of
    them) zero-extended."""
    if tokens.dtype == torch.int32:
        return tokens
    if tokens.dtype == torch.int16:
        return tokens.to(torch.int32) & 0xFFFF
    if tokens.dtype == torch.uint16:
        return tokens.view(torch.int16).to(torch.int32) & 0xFFFF
    raise TypeError(f"tokens must be int32 or 16-bit, got {tokens.dtype}")


def ref_pad_tokens(tokens: torch.Tensor, offsets: torch.Tensor, seq_len: int, pad_id: int = 0,
                   position_dtype=torch.int64):
    offs = offsets.to("cpu", torch.int64).tolist()
    b = len(offs) - 1
    t = widen_tokens(tokens.cpu())
    out = torch.full((b, seq_len), pad_id, dtype=torch.int32)
    mask = torch.zeros((b, seq_len), dtype=torch.uint8)
    pos = torch.zeros((b, seq_len), dtype=position_dtype)
    for i in range(b):
        n = min(offs[i + 1] - offs[i], seq_len)
        if n > 0:
            out[i, :n] = t[offs[i]:offs[i] + n]
            mask[i, :n] = 1
            pos[i, :n] = torch.arange(n, dtype=position_dtype)
    return out, mask, pos


def ref_token_labels(input_ids: torch.Tensor, attention_mask: torch.Tensor, segment_ids: torch.Tensor | None = None,
                     ignore_index: int = -100) -> torch.Tensor:
    """Next-token labels of a token batch (int64 [R, S], what ``cross_entropy(..., ignore_index=ignore_index)``
    takes), with torch ops on the batch's device -- the definition the kernels' ``labels=True`` implements::

        labels[r, p] = input_ids[r, p + 1]   if p + 1 < S and attention_mask[r, p + 1] == 1
                                             and (pad mode or segment_ids[r, p + 1] == segment_ids[r, p])
                     = ignore_index          otherwise

    ``segment_ids`` None: pad mode. So the last position of a row (a pad row truncated at S included), the last
    token of every segment (each ``seq_len`` chunk of an over-long packed sequence is its own segment), a
    one-token segment, and every padding position and padding row are ``ignore_index``."""
    ids = input_ids.to(torch.int64)
    lab = torch.full_like(ids, int(ignore_index))
    if ids.shape[-1] > 1:
        ok = attention_mask[..., 1:] != 0
        if segment_ids is not None:
            ok = ok & (segment_ids[..., 1:] == segment_ids[..., :-1])
        lab[..., :-1] = torch.where(ok, ids[..., 1:], lab[..., :-1])
    return lab


def check_ignore_index(labels: bool, ignore_index: int) -> int:
    """The checked ``ignore_index`` (the kernels carry it as an int32)."""
    ignore_index = int(ignore_index)
    if labels and not -(1 << 31) <= ignore_index < (1 << 31):
        raise ValueError(f"ignore_index={ignore_index} does not fit int32")
    return ignore_index


def pad_tokens(tokens: torch.Tensor, offsets: torch.Tensor, seq_len: int, pad_id: int = 0,
               position_dtype=torch.int64, stream=None, labels: bool = False, ignore_index: int = -100):
    """Ragged token stream (int32, or 16-bit ids widened by the kernel) + [B+1] int64 offsets ->
    (tokens [B,S] i32, mask u8 [B,S], position ids [B,S]); ``labels=True`` appends the next-token labels (int64
    [B,S], ``ref_token_labels``), written by the same kernel."""
    if (tokens.dtype != torch.int32 and tokens.dtype not in _TOK16) or offsets.dtype != torch.int64:
        raise TypeError("tokens must be int32 / 16-bit and offsets int64")
    ignore_index = check_ignore_index(labels, ignore_index)
    if not tokens.is_cuda:
        r = ref_pad_tokens(tokens, offsets, seq_len, pad_id, position_dtype)
        return (*r, ref_token_labels(r[0], r[1], None, ignore_index)) if labels else r
    b = offsets.numel() - 1
    dev = tokens.device
    out = torch.empty((b, seq_len), dtype=torch.int32, device=dev)
    mask = torch.empty((b, seq_len), dtype=torch.uint8, device=dev)
    pos = torch.empty((b, seq_len), dtype=position_dtype, device=dev)
    lab = torch.empty((b, seq_len), dtype=torch.int64, device=dev) if labels else None
    _native.hip().pad_pack_tokens(
        tokens=tokens.data_ptr(), offsets=offsets.data_ptr(), row_start=0, row_end=0, seg_offsets=0, n_seg=0,
        out_tokens=out.data_ptr(), attn_mask=mask.data_ptr(), position_ids=pos.data_ptr(),
        pos_is_i64=position_dtype == torch.int64, segment_ids=0, cu_seqlens_out=0, rows=b, seq_len=seq_len,
        pad_id=pad_id, mode=0, stream=_stream_handle(stream), tok16=tokens.dtype in _TOK16,
        labels=lab.data_ptr() if labels else 0, ignore_index=ignore_index)
    return (out, mask, pos, lab) if labels else (out, mask, pos)


def pack_plan(seq_offsets: np.ndarray, seq_len: int, max_rows: int | None = None):
    """Greedy in-order packing of sequences into rows of ``seq_len`` tokens (native C++).

    Sequences longer than ``seq_len`` are split into ``seq_len`` chunks (each
    chunk restarts its position ids). Returns (row_start, row_end, seg_offsets)
    int64 arrays: row r holds flat tokens [row_start[r], row_end[r]);
    seg_offsets are the (split) sequence starts plus the end. ``max_rows``
    truncates the plan (reference implementation).
    """
    offs = np.ascontiguousarray(seq_offsets, dtype=np.int64)
    if max_rows is not None:
        return ref_pack_plan(offs, seq_len, max_rows)
    n = len(offs) - 1
    lens = np.diff(offs)
    max_segs = int(np.sum(-(-lens // seq_len))) if n > 0 else 0
    rs = np.empty(max(max_segs, 1), np.int64)
    re_ = np.empty(max(max_segs, 1), np.int64)
    so = np.empty(max_segs + 1, np.int64)
    n_rows, n_seg = _native.runtime().pack_plan(offs.ctypes.data, n, int(seq_len), rs.ctypes.data, re_.ctypes.data,
                                               max(max_segs, 1), so.ctypes.data, max_segs)
    return rs[:n_rows].copy(), re_[:n_rows].copy(), so[: n_seg + 1].copy()


def ref_pack_plan(seq_offsets: np.ndarray, seq_len: int, max_rows: int | None = None):
    """Pure-Python reference of ``pack_plan``.

    Sequences longer than ``seq_len`` are split into ``seq_len`` chunks (each
    chunk restarts its position ids). Returns (row_start, row_end, seg_offsets)
    int64 arrays: row r holds flat tokens [row_start[r], row_end[r]);
    seg_offsets are the (split) sequence starts plus the end.
    """
    offs = np.asarray(seq_offsets, dtype=np.int64)
    segs = []
    for i in range(len(offs) - 1):
        s, e = int(offs[i]), int(offs[i + 1])
        while e - s > seq_len:
            segs.append((s, s + seq_len))
            s += seq_len
        if e > s:
            segs.append((s, e))
    row_start, row_end = [], []
    cur_s, cur_e = None, None
    for s, e in segs:
        if cur_s is None:
            cur_s, cur_e = s, e
        elif e - cur_s <= seq_len and s == cur_e:
            cur_e = e
        else:
            row_start.append(cur_s)
            row_end.append(cur_e)
            cur_s, cur_e = s, e
        if max_rows is not None and len(row_start) >= max_rows:
            break
    if cur_s is not None and (max_rows is None or len(row_start) < max_rows):
        row_start.append(cur_s)
        row_end.append(cur_e)
    seg_offsets = np.array([s for s, _ in segs] + ([segs[-1][1]] if segs else [0]), dtype=np.int64)
    return np.array(row_start, dtype=np.int64), np.array(row_end, dtype=np.int64), seg_offsets


def ref_pack_tokens(tokens, row_start, row_end, seg_offsets, seq_len, pad_id=0, position_dtype=torch.int64,
                    fill_rows: int = 0):
    """CPU reference of pack mode; ``fill_rows`` > packed rows: padding rows up to that fixed row count."""
    t = widen_tokens(tokens.cpu())
    rs, re_, so = (np.asarray(a) for a in (row_start, row_end, seg_offsets))
    r = max(len(rs), int(fill_rows))
    out = torch.full((r, seq_len), pad_id, dtype=torch.int32)
    mask = torch.zeros((r, seq_len), dtype=torch.uint8)
    pos = torch.zeros((r, seq_len), dtype=position_dtype)
    seg = torch.full((r, seq_len), -1, dtype=torch.int32)
    for i in range(len(rs)):
        n = min(int(re_[i] - rs[i]), seq_len)
        g = np.arange(rs[i], rs[i] + n)
        sidx = np.searchsorted(so, g, side="right") - 1
        out[i, :n] = t[rs[i]:rs[i] + n]
        mask[i, :n] = 1
        pos[i, :n] = torch.from_numpy(g - so[sidx]).to(position_dtype)
        seg[i, :n] = torch.from_numpy(sidx.astype(np.int32))
    return out, mask, pos, seg


def pack_capacity(n_seq: int, n_tokens: int, seq_len: int) -> tuple[int, int]:
    """(max segments, max rows) that in-order packing of ``n_seq`` sequences holding at most ``n_tokens``
    tokens can produce: each sequence splits into ceil(len / S) segments (<= n_seq + n_tokens // S in total),
    and two consecutive rows together hold more than S tokens (else the greedy pass would have merged them),
    so rows <= 2 * ceil(n_tokens / S) + 1."""
    S = int(seq_len)
    max_segs = int(n_seq) + int(n_tokens) // S
    max_rows = min(max_segs, 2 * (-(-int(n_tokens) // S)) + 1)
    return max_segs, max(max_rows, 0)


def pack_tokens_device(tokens: torch.Tensor, offsets: torch.Tensor, seq_len: int, pad_id: int = 0,
                       position_dtype=torch.int64, max_rows: int | None = None, stream=None, labels: bool = False,
                       ignore_index: int = -100) -> dict:
    """Pack with the plan built ON THE DEVICE: two launches (``pack_plan_device``, then the pack kernel
    reading the plan's row count from device memory), no host round trip, static output shapes.

    ``offsets`` is the [B+1] int64 offsets tensor on the tokens' device. Outputs have ``max_rows`` rows
    (default: ``pack_capacity`` of the token buffer, an upper bound the plan cannot exceed); rows past the
    plan's are padding (pad_id, mask 0, position 0, segment -1). Returns a dict: ``input_ids``,
    ``attention_mask``, ``position_ids``, ``segment_ids``, ``cu_seqlens`` (int32, capacity max_segs + 1; only
    the first n_seg + 1 entries are written), ``counts`` (device int64 [n_rows, n_seg]; n_rows = -1 if max_rows
    was too small, every row then padding). ``labels=True`` adds ``labels`` (``ref_token_labels``; all
    ``ignore_index`` for an overflowed plan). Reference of the plan: ``pack_plan`` (host, runtime/arena.cpp).
    Graph-capturable: nothing in it synchronises with the host.
    """
    ignore_index = check_ignore_index(labels, ignore_index)
    if (tokens.dtype != torch.int32 and tokens.dtype not in _TOK16) or offsets.dtype != torch.int64:
        raise TypeError("tokens must be int32 / 16-bit and offsets int64")
    n = offsets.numel() - 1
    if n < 0:
        raise ValueError("offsets needs at least one entry")
    S = int(seq_len)
    max_segs, cap_rows = pack_capacity(n, tokens.numel(), S)
    R = cap_rows if max_rows is None else int(max_rows)
    dev = tokens.device
    if not tokens.is_cuda:  # host reference: the same outputs from the host plan
        rs, re_, so = ref_pack_plan(offsets.cpu().numpy(), S)
        ok = len(rs) <= R
        out, mask, pos, seg = ref_pack_tokens(tokens, rs[:R] if ok else rs[:0], re_[:R] if ok else re_[:0], so, S,
                                              pad_id, position_dtype, fill_rows=R)
        cu = torch.zeros(max_segs + 1, dtype=torch.int32)
        cu[:len(so)] = torch.from_numpy(so.astype(np.int32))
        counts = torch.tensor([len(rs) if ok else -1, len(so) - 1], dtype=torch.int64)
        r = {"input_ids": out[:R], "attention_mask": mask[:R], "position_ids": pos[:R], "segment_ids": seg[:R],
             "cu_seqlens": cu, "counts": counts}
        if labels:
            r["labels"] = ref_token_labels(r["input_ids"], r["attention_mask"], r["segment_ids"], ignore_index)
        return r
    if not offsets.is_cuda or offsets.device != dev:
        raise ValueError("offsets must be on the tokens' device (use pack_tokens for host offsets)")
    h = _native.hip()
    offsets = offsets.contiguous()
    # one allocation for the plan, its scratch and the five outputs (16-byte aligned regions)
    pb = 8 if position_dtype == torch.int64 else 4
    sizes = [8 * (max_segs + 1), 8 * max(R, 1), 8 * max(R, 1), 16, 4 * h.pack_plan_scratch_ints(max_segs, R),
             4 * R * S, R * S, pb * R * S, 4 * R * S, 4 * (max_segs + 1), 8 * R * S if labels else 0]
    offs_b = [0]
    for n_b in sizes:
        offs_b.append(offs_b[-1] + -(-n_b // 16) * 16)
    whole = torch.empty(offs_b[-1], dtype=torch.uint8, device=dev)
    reg = [whole[a:a + n_b] for a, n_b in zip(offs_b, sizes)]
    so, rs, re_, counts = (r.view(torch.int64) for r in reg[:4])
    scratch = reg[4].view(torch.int32)
    out = reg[5].view(torch.int32).view(R, S)
    mask = reg[6].view(R, S)
    pos = reg[7].view(position_dtype).view(R, S)
    seg = reg[8].view(torch.int32).view(R, S)
    cu = reg[9].view(torch.int32)
    lab = reg[10].view(torch.int64).view(R, S) if labels else None
    sh = _stream_handle(stream)
    h.pack_plan_device(offsets=offsets.data_ptr(), n=n, seq_len=S, max_segs=max_segs, max_rows=R,
                       seg_offsets=so.data_ptr(), row_start=rs.data_ptr(), row_end=re_.data_ptr(),
                       counts=counts.data_ptr(), scratch=scratch.data_ptr(), stream=sh)
    if R > 0:
        h.pad_pack_tokens(
            tokens=tokens.data_ptr(), offsets=0, row_start=rs.data_ptr(), row_end=re_.data_ptr(),
            seg_offsets=so.data_ptr(), n_seg=0, out_tokens=out.data_ptr(), attn_mask=mask.data_ptr(),
            position_ids=pos.data_ptr(), pos_is_i64=position_dtype == torch.int64, segment_ids=seg.data_ptr(),
            cu_seqlens_out=cu.data_ptr(), rows=0, seq_len=S, pad_id=pad_id, mode=1, stream=sh, fill_rows=R,
            dev_counts=counts.data_ptr(), tok16=tokens.dtype in _TOK16, labels=lab.data_ptr() if labels else 0,
            ignore_index=ignore_index)
    else:  # no rows to launch over: the (empty) plan's cu_seqlens is the single 0
        cu[:1].zero_()
    r = {"input_ids": out, "attention_mask": mask, "position_ids": pos, "segment_ids": seg, "cu_seqlens": cu,
         "counts": counts}
    if labels:
        r["labels"] = lab
    return r


def pack_tokens(tokens: torch.Tensor, seq_offsets, seq_len: int, pad_id: int = 0, position_dtype=torch.int64,
                stream=None, labels: bool = False, ignore_index: int = -100):
    """Pack a ragged token stream into rows of ``seq_len`` (varlen-attention layout).

    Returns (tokens [R,S] i32, mask [R,S] u8, position_ids [R,S], segment_ids [R,S] i32 (-1 = pad),
    cu_seqlens [n_seg+1] i32 over the unpadded stream ``tokens[mask.bool()]``); ``labels=True`` appends the
    next-token labels (int64 [R,S], ``ref_token_labels``), written by the same kernel.

    Offsets already on the tokens' GPU: the plan is built on the device (``pack_tokens_device``) and the
    one host synchronisation is the read of the row count that sizes the result. Host offsets: the host
    plan (native ``pack_plan``), uploaded with the launch.
    """
    ignore_index = check_ignore_index(labels, ignore_index)
    if tokens.is_cuda and torch.is_tensor(seq_offsets) and seq_offsets.device == tokens.device:
        r = pack_tokens_device(tokens, seq_offsets.to(torch.int64), seq_len, pad_id, position_dtype, stream=stream,
                               labels=labels, ignore_index=ignore_index)
        n_rows, n_seg = (int(v) for v in r["counts"].cpu())
        if n_rows < 0:  # cannot happen within pack_capacity; kept loud
            raise RuntimeError(f"device pack plan overflowed ({n_seg} segments)")
        return (r["input_ids"][:n_rows], r["attention_mask"][:n_rows], r["position_ids"][:n_rows],
                r["segment_ids"][:n_rows], r["cu_seqlens"][:n_seg + 1],
                *((r["labels"][:n_rows],) if labels else ()))
    rs, re_, so = pack_plan(np.asarray(seq_offsets.cpu() if torch.is_tensor(seq_offsets) else seq_offsets),
                            seq_len)
    cu = torch.from_numpy(so.astype(np.int32))
    if not tokens.is_cuda:
        r = ref_pack_tokens(tokens, rs, re_, so, seq_len, pad_id, position_dtype)
        return (*r, cu, *((ref_token_labels(r[0], r[1], r[3], ignore_index),) if labels else ()))
    dev = tokens.device
    rs_d, re_d, so_d = (torch.from_numpy(a).to(dev, non_blocking=False) for a in (rs, re_, so))
    r = len(rs)
    out = torch.empty((r, seq_len), dtype=torch.int32, device=dev)
    mask = torch.empty((r, seq_len), dtype=torch.uint8, device=dev)
    pos = torch.empty((r, seq_len), dtype=position_dtype, device=dev)
    seg = torch.empty((r, seq_len), dtype=torch.int32, device=dev)
    lab = torch.empty((r, seq_len), dtype=torch.int64, device=dev) if labels else None
    _native.hip().pad_pack_tokens(
        tokens=tokens.data_ptr(), offsets=0, row_start=rs_d.data_ptr(), row_end=re_d.data_ptr(),
        seg_offsets=so_d.data_ptr(), n_seg=len(so) - 1, out_tokens=out.data_ptr(), attn_mask=mask.data_ptr(),
        position_ids=pos.data_ptr(), pos_is_i64=position_dtype == torch.int64, segment_ids=seg.data_ptr(),
        cu_seqlens_out=0, rows=r, seq_len=seq_len, pad_id=pad_id, mode=1, stream=_stream_handle(stream),
        tok16=tokens.dtype in _TOK16, labels=lab.data_ptr() if labels else 0, ignore_index=ignore_index)
    return (out, mask, pos, seg, so_d.to(torch.int32), *((lab,) if labels else ()))


# ------------------------------------------------- tokens out of an HBM corpus
def _align16(n: int) -> int:
    return -(-int(n) // 16) * 16


def token_output_bytes(rows: int, seq_len: int, n_seg: int | None = None, position_dtype=torch.int64,
                       labels: bool = False) -> int:
    """Bytes of the one allocation that ``carve_token_outputs`` cuts a [rows, seq_len] token batch from
    (``n_seg`` None: pad mode, no segment ids and no cu_seqlens; ``labels``: with the int64 next-token labels)."""
    # per-step host code of every token path: (x + 15) & -16 is _align16(x), written out to spare the calls
    n = int(rows) * int(seq_len)
    pos_b = (8 if position_dtype == torch.int64 else 4) * n
    ids_b = (4 * n + 15) & -16  # input ids, and the segment ids
    total = ((pos_b + 15) & -16) + ids_b + ((n + 15) & -16)  # position ids, input ids, mask
    if n_seg is not None:
        total += ((4 * (n_seg + 1) + 15) & -16) + ids_b  # cu_seqlens [n_seg + 1] i32, segment ids
    if labels:
        total += (8 * n + 15) & -16
    return total


def carve_token_outputs(whole: torch.Tensor, rows: int, seq_len: int, n_seg: int | None = None,
                        position_dtype=torch.int64, labels: bool = False):
    """(input_ids, attention_mask, position_ids, segment_ids | None, cu_seqlens | None) as views of the uint8
    buffer ``whole``: position ids, cu_seqlens, input ids, segment ids, mask, every region starting 16-byte
    aligned. ``labels=True`` appends the labels view (int64 [rows, seq_len]) to the tuple, carved behind the
    mask; the other views stay where they are without it. The one definition of a token batch's allocation:
    ``collate_token_window``, the indexed ops and the resident loader all carve with it."""
    R, S = int(rows), int(seq_len)
    n = R * S
    pos_b = (8 if position_dtype == torch.int64 else 4) * n
    ids_b = 4 * n
    ids_a = (ids_b + 15) & -16  # _align16, written out as in token_output_bytes
    pos = whole[:pos_b].view(position_dtype).view(R, S)
    o = (pos_b + 15) & -16
    cu = seg = None
    if n_seg is not None:
        cu_b = 4 * (n_seg + 1)
        cu = whole[o:o + cu_b].view(torch.int32)
        o += (cu_b + 15) & -16
    ids = whole[o:o + ids_b].view(torch.int32).view(R, S)
    o += ids_a
    if n_seg is not None:
        seg = whole[o:o + ids_b].view(torch.int32).view(R, S)
        o += ids_a
    mask = whole[o:o + n].view(R, S)
    if labels:
        o += (n + 15) & -16
        return ids, mask, pos, seg, cu, whole[o:o + 8 * n].view(torch.int64).view(R, S)
    return ids, mask, pos, seg, cu


def _token_out_buffer(out, need: int, dev) -> torch.Tensor:
    if out is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if (not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()
            or out.numel() < need or out.data_ptr() % 16):
        raise ValueError(f"out must be a contiguous 16-byte aligned uint8 device buffer of >= {need} bytes")
    return out[:need]


def segment_sources(src_start: np.ndarray, offsets: np.ndarray, seg_offsets: np.ndarray, n_seg: int) -> np.ndarray:
    """``seg_src`` [n_seg]: the corpus element of each segment's first token, for sequences that start at corpus
    elements ``src_start`` [n] and at ``offsets`` [n + 1] of the virtual flat stream the plan's ``seg_offsets``
    refer to. A segment is a piece of one sequence: the last one that starts at or before it (an empty sequence
    shares its start with the next one and holds no segment)."""
    so = seg_offsets[:n_seg]
    q = np.searchsorted(offsets, so, side="right") - 1
    return src_start[q] + (so - offsets[q])


def _indexed_args(corpus, corpus_offsets, idx, position_dtype):
    if position_dtype not in (torch.int64, torch.int32):
        raise TypeError("position_dtype must be int64 or int32")
    if not isinstance(corpus, torch.Tensor) or (corpus.dtype != torch.int32 and corpus.dtype not in _TOK16):
        raise TypeError("corpus must be a flat int32 / 16-bit token tensor")
    if not corpus.is_contiguous():
        raise ValueError("corpus must be contiguous")
    flat, start, dofs = _ragged_args(corpus, corpus_offsets, idx)
    if int(dofs[-1]) > 0x7FFFFFFF:
        raise ValueError(f"{int(dofs[-1])} tokens in one batch overflow int32 cu_seqlens")
    return flat, np.ascontiguousarray(start, dtype=np.int64), dofs


def _upload_words(words: np.ndarray, dev, stream):
    handle, stream = _stream_pair(stream, dev)
    with torch.cuda.stream(stream):  # None: the current stream. The descriptor is allocated and copied on it
        desc = torch.from_numpy(words).to(dev)  # a pageable copy: complete for the host on return
    return desc, handle, stream


def pad_tokens_indexed(corpus: torch.Tensor, corpus_offsets, idx, seq_len: int, pad_id: int = 0,
                       position_dtype=torch.int64, out: torch.Tensor | None = None, stream=None,
                       labels: bool = False, ignore_index: int = -100):
    """``pad_tokens`` of sequences ``idx`` of a corpus that lives in HBM, in one pass: ``corpus`` is the flat
    device tensor (int32 or 16-bit ids), sequence i = ``corpus[corpus_offsets[i]:corpus_offsets[i + 1]]``;
    ``corpus_offsets`` and ``idx`` live on the host. The gathered stream is never materialised (the
    ``pad_pack_tokens_indexed`` kernel reads every token from the corpus). Returns (tokens [B,S] i32, mask u8
    [B,S], position ids [B,S]); ``out``: a uint8 device buffer the three are carved from
    (``token_output_bytes`` / ``carve_token_outputs``). ``labels=True`` appends the next-token labels (int64
    [B,S], ``ref_token_labels``), written by the same kernel and carved from the same buffer. A CPU corpus takes
    the reference path (``ref_gather_ragged`` + ``ref_pad_tokens`` + ``ref_token_labels``)."""
    flat, start, dofs = _indexed_args(corpus, corpus_offsets, idx, position_dtype)
    ignore_index = check_ignore_index(labels, ignore_index)
    S = int(seq_len)
    if S <= 0:
        raise ValueError("seq_len must be > 0")
    if not flat.is_cuda:
        tokens, offs = ref_gather_ragged(flat, corpus_offsets, idx)
        r = ref_pad_tokens(tokens, offs, S, pad_id, position_dtype)
        return (*r, ref_token_labels(r[0], r[1], None, ignore_index)) if labels else r
    n, dev = int(start.size), flat.device
    words = np.concatenate([start, dofs])  # one descriptor: src_start [n], offsets [n + 1]
    desc, handle, stream = _upload_words(words, dev, stream)
    with torch.cuda.stream(stream):
        whole = _token_out_buffer(out, token_output_bytes(n, S, None, position_dtype, labels), dev)
    ids, mask, pos, _, _, *lab = carve_token_outputs(whole, n, S, None, position_dtype, labels)
    base = desc.data_ptr()
    _native.hip().pad_pack_tokens_indexed(
        corpus=flat.data_ptr(), corpus_elems=flat.numel(), src_start=base, seg_src=0, offsets=base + 8 * n,
        row_start=0, row_end=0, seg_offsets=0, n_seg=0, out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(),
        position_ids=pos.data_ptr(), pos_is_i64=position_dtype == torch.int64, segment_ids=0, cu_seqlens_out=0,
        rows=n, seq_len=S, pad_id=pad_id, mode=0, stream=handle, tok16=flat.dtype in _TOK16,
        labels=lab[0].data_ptr() if labels else 0, ignore_index=ignore_index)
    return (ids, mask, pos, *lab)


def pack_tokens_indexed(corpus: torch.Tensor, corpus_offsets, idx, seq_len: int, pad_id: int = 0,
                        position_dtype=torch.int64, fill_rows: int = 0, out: torch.Tensor | None = None, stream=None,
                        labels: bool = False, ignore_index: int = -100):
    """``pack_tokens`` of sequences ``idx`` of a corpus that lives in HBM, in one pass (see
    ``pad_tokens_indexed``): the host computes the sequences' running offsets, the native ``pack_plan`` and each
    segment's corpus element, uploads them as one descriptor, and the ``pad_pack_tokens_indexed`` kernel packs
    straight out of the corpus. Returns (tokens [R,S] i32, mask [R,S] u8, position_ids [R,S], segment_ids [R,S]
    i32 (-1 = pad), cu_seqlens [n_seg+1] i32); ``fill_rows`` > packed rows: padding rows up to that count;
    ``out``: a uint8 device buffer the five are carved from. ``labels=True`` appends the next-token labels (int64
    [R,S], ``ref_token_labels``; padding rows all ``ignore_index``), written by the same kernel and carved from
    the same buffer. A CPU corpus takes the reference path (``ref_gather_ragged`` + ``ref_pack_plan`` +
    ``ref_pack_tokens`` + ``ref_token_labels``)."""
    flat, start, dofs = _indexed_args(corpus, corpus_offsets, idx, position_dtype)
    ignore_index = check_ignore_index(labels, ignore_index)
    S = int(seq_len)
    if S <= 0:
        raise ValueError("seq_len must be > 0")
    if not flat.is_cuda:
        tokens, offs = ref_gather_ragged(flat, corpus_offsets, idx)
        rs, re_, so = ref_pack_plan(offs.numpy(), S)
        r = ref_pack_tokens(tokens, rs, re_, so, S, pad_id, position_dtype, fill_rows=fill_rows)
        return (*r, torch.from_numpy(so.astype(np.int32)),
                *((ref_token_labels(r[0], r[1], r[3], ignore_index),) if labels else ()))
    n, dev = int(start.size), flat.device
    lens = np.diff(dofs)
    cap = max(int(np.sum(-(-lens // S))) if n else 0, 1)  # segments (>= rows) of this batch
    # one descriptor: src_start [n], offsets [n + 1], row_start [cap], row_end [cap], seg_offsets [cap + 1],
    # seg_src [cap]
    words = np.zeros(2 * n + 1 + 4 * cap + 1, dtype=np.int64)
    words[:n], words[n:2 * n + 1] = start, dofs
    o_rs, o_re, o_so, o_ss = 2 * n + 1, 2 * n + 1 + cap, 2 * n + 1 + 2 * cap, 2 * n + 2 + 3 * cap
    n_rows, n_seg = _native.runtime().pack_plan(words[n:].ctypes.data, n, S, words[o_rs:].ctypes.data,
                                                words[o_re:].ctypes.data, cap, words[o_so:].ctypes.data, cap)
    words[o_ss:o_ss + n_seg] = segment_sources(start, dofs, words[o_so:], n_seg)
    R = max(int(n_rows), int(fill_rows))
    desc, handle, stream = _upload_words(words, dev, stream)
    with torch.cuda.stream(stream):
        whole = _token_out_buffer(out, token_output_bytes(R, S, n_seg, position_dtype, labels), dev)
    ids, mask, pos, seg, cu, *lab = carve_token_outputs(whole, R, S, n_seg, position_dtype, labels)
    base = desc.data_ptr()
    _native.hip().pad_pack_tokens_indexed(
        corpus=flat.data_ptr(), corpus_elems=flat.numel(), src_start=base, seg_src=base + 8 * o_ss, offsets=0,
        row_start=base + 8 * o_rs, row_end=base + 8 * o_re, seg_offsets=base + 8 * o_so, n_seg=n_seg,
        out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(), position_ids=pos.data_ptr(),
        pos_is_i64=position_dtype == torch.int64, segment_ids=seg.data_ptr(), cu_seqlens_out=cu.data_ptr(),
        rows=n_rows, seq_len=S, pad_id=pad_id, mode=1, stream=handle, fill_rows=int(fill_rows),
        tok16=flat.dtype in _TOK16, labels=lab[0].data_ptr() if labels else 0, ignore_index=ignore_index)
    return (ids, mask, pos, seg, cu, *lab)


# ------------------------------- tokens out of an HBM corpus, planned on the device
def device_plan_bytes(n: int, max_segs: int | None = None, max_rows: int = 0, ffd: bool = False) -> int:
    """Bytes of the plan arrays the device-planned ops keep between their launches (``max_segs`` None: pad mode):
    src_start [n], offsets [n + 1], and in pack mode seg_src [max_segs], seg_offsets [max_segs + 1], row_start /
    row_end [max_rows] and the plan kernel's scratch; with ``ffd`` (pack mode) the index [n] and the three counts of
    ``token_ffd_order`` behind them. Nothing a caller holds lives here."""
    total = _align16(8 * n) + _align16(8 * (n + 1))
    if max_segs is not None:
        total += (_align16(8 * max_segs) + _align16(8 * (max_segs + 1)) + 2 * _align16(8 * max_rows)
                  + _align16(4 * (2 * (max_segs + 1) + max_rows + 1)))  # == pack_plan_scratch_ints
        if ffd:
            total += _align16(8 * n) + 32
    return total


def device_batch_bytes(rows: int, seq_len: int, max_segs: int | None = None, position_dtype=torch.int64,
                       labels: bool = False) -> int:
    """Bytes of what a device-planned batch hands to its caller: ``token_output_bytes`` (``cu_seqlens`` of
    capacity ``max_segs`` + 1 in pack mode; ``labels``: with the next-token labels) and the four int64 counts
    behind it."""
    return token_output_bytes(rows, seq_len, max_segs, position_dtype, labels) + 32


def launch_device_plan(plan_ptr: int, whole: torch.Tensor, *, corpus_ptr: int, corpus_elems: int, tok16: bool,
                       corpus_offsets_ptr: int, n_corpus: int, selector: dict, n: int, seq_len: int, pad_id: int,
                       pack: bool, max_segs: int = 0, max_rows: int = 0, position_dtype=torch.int64,
                       stream: int = 0, labels: bool = False, ignore_index: int = -100, ffd: bool = False) -> dict:
    """The launches of one device-planned batch on raw stream ``stream``: descriptor, (pack mode) plan, pack; with
    ``ffd`` (pack mode, ``device_plan_bytes(..., ffd=True)``) ``token_ffd_order`` in front, and the descriptor runs
    on its index. ``plan_ptr``: ``device_plan_bytes`` of 16-byte aligned device memory for the plan arrays; ``whole``:
    ``device_batch_bytes`` of uint8 device memory the outputs and the counts are carved from; ``selector``: the
    ``mode / idx / base / keys / n_domain / half_bits`` of a ``RowIndex``. Nothing here allocates, copies or
    synchronises. Returns the dict of ``pack_tokens_indexed_device`` / ``pad_tokens_indexed_device``
    (``labels=True``: with ``"labels"``, written by the pack launch)."""
    h = _native.hip()
    n, S, R, M = int(n), int(seq_len), int(max_rows), int(max_segs)
    ignore_index = check_ignore_index(labels, ignore_index)
    o_src = plan_ptr
    o_off = o_src + _align16(8 * n)
    o_end = o_off + _align16(8 * (n + 1))
    i64 = position_dtype == torch.int64
    if not pack:
        out_b = token_output_bytes(n, S, None, position_dtype, labels)
        ids, mask, pos, _, _, *lab = carve_token_outputs(whole, n, S, None, position_dtype, labels)
        counts = whole[out_b:out_b + 32].view(torch.int64)
        h.token_batch_descriptor(corpus_offsets=corpus_offsets_ptr, n_corpus=n_corpus, n=n, seq_len=S, max_segs=0,
                                 src_start=o_src, offsets=o_off, seg_src=0, counts=counts.data_ptr(),
                                 pad_counts=True, stream=stream, **selector)
        h.pad_pack_tokens_indexed(
            corpus=corpus_ptr, corpus_elems=corpus_elems, src_start=o_src, seg_src=0, offsets=o_off, row_start=0,
            row_end=0, seg_offsets=0, n_seg=0, out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(),
            position_ids=pos.data_ptr(), pos_is_i64=i64, segment_ids=0, cu_seqlens_out=0, rows=n, seq_len=S,
            pad_id=pad_id, mode=0, stream=stream, tok16=tok16, labels=lab[0].data_ptr() if labels else 0,
            ignore_index=ignore_index)
        r = {"input_ids": ids, "attention_mask": mask, "position_ids": pos, "counts": counts}
    else:
        o_ss = o_end
        o_so = o_ss + _align16(8 * M)
        o_rs = o_so + _align16(8 * (M + 1))
        o_re = o_rs + _align16(8 * R)
        o_scr = o_re + _align16(8 * R)
        out_b = token_output_bytes(R, S, M, position_dtype, labels)
        ids, mask, pos, seg, cu, *lab = carve_token_outputs(whole, R, S, M, position_dtype, labels)
        counts = whole[out_b:out_b + 32].view(torch.int64)
        c_ptr = counts.data_ptr()
        if ffd and n:  # n = 0: nothing to order (the descriptor reads no index)
            o_idx = o_scr + _align16(4 * (2 * (M + 1) + R + 1))
            h.token_ffd_order(corpus_offsets=corpus_offsets_ptr, n_corpus=n_corpus, n=n, seq_len=S, index_out=o_idx,
                              counts=o_idx + _align16(8 * n), stream=stream, **selector)
            selector = dict(mode=1, idx=o_idx, base=0, keys=[0] * 6, n_domain=1, half_bits=1)
        h.token_batch_descriptor(corpus_offsets=corpus_offsets_ptr, n_corpus=n_corpus, n=n, seq_len=S, max_segs=M,
                                 src_start=o_src, offsets=o_off, seg_src=o_ss, counts=c_ptr, pad_counts=False,
                                 stream=stream, **selector)
        h.pack_plan_device(offsets=o_off, n=n, seq_len=S, max_segs=M, max_rows=R, seg_offsets=o_so, row_start=o_rs,
                           row_end=o_re, counts=c_ptr, scratch=o_scr, stream=stream)
        h.pad_pack_tokens_indexed(
            corpus=corpus_ptr, corpus_elems=corpus_elems, src_start=o_src, seg_src=o_ss, offsets=0, row_start=o_rs,
            row_end=o_re, seg_offsets=o_so, n_seg=0, out_tokens=ids.data_ptr(), attn_mask=mask.data_ptr(),
            position_ids=pos.data_ptr(), pos_is_i64=i64, segment_ids=seg.data_ptr(), cu_seqlens_out=cu.data_ptr(),
            rows=0, seq_len=S, pad_id=pad_id, mode=1, stream=stream, fill_rows=R, tok16=tok16, dev_counts=c_ptr,
            cu_cap=M, labels=lab[0].data_ptr() if labels else 0, ignore_index=ignore_index)
        r = {"input_ids": ids, "attention_mask": mask, "position_ids": pos, "segment_ids": seg, "cu_seqlens": cu,
             "counts": counts}
    if labels:
        r["labels"] = lab[0]
    return r


def _selection_args(corpus_offsets, index, perm, base, count) -> tuple[torch.Tensor, int]:
    """Checked (flat offsets, n) of a selection of corpus sequences: a device ``index``, or positions ``[base, base +
    count)`` of ``perm`` or of the identity."""
    offs = corpus_offsets.reshape(-1)
    if offs.numel() < 1:
        raise ValueError("corpus_offsets needs at least one entry")
    if index is not None and perm is not None:
        raise ValueError("give either index or perm, not both")
    if index is not None and (index.dtype != torch.int64 or index.device != corpus_offsets.device
                              or not index.is_contiguous()):
        raise ValueError("index must be a contiguous int64 tensor on the corpus's device")
    if index is not None and count is not None and int(count) != index.numel():
        raise ValueError("count does not match the index")
    n_corpus = offs.numel() - 1
    if index is not None:
        n = index.numel()
    elif count is not None:
        n = int(count)
    else:
        n = (perm.n if perm is not None else n_corpus) - int(base)
    if n < 0 or (index is None and int(base) < 0):
        raise ValueError("negative base or count")
    if perm is not None and (int(base) + n > perm.n or perm.n > n_corpus):
        raise IndexError("perm positions out of range, or a permutation domain larger than the corpus")
    if index is None and perm is None and int(base) + n > n_corpus:
        raise IndexError("identity rows out of range")
    return offs, n


def _device_plan_args(corpus, corpus_offsets, index, perm, base, count, seq_len, position_dtype):
    """Checked (flat corpus, offsets, n) of a device-planned op."""
    if position_dtype not in (torch.int64, torch.int32):
        raise TypeError("position_dtype must be int64 or int32")
    if not isinstance(corpus, torch.Tensor) or (corpus.dtype != torch.int32 and corpus.dtype not in _TOK16):
        raise TypeError("corpus must be a flat int32 / 16-bit token tensor")
    if not isinstance(corpus_offsets, torch.Tensor) or corpus_offsets.dtype != torch.int64:
        raise TypeError("corpus_offsets must be an int64 tensor")
    if not corpus.is_contiguous() or not corpus_offsets.is_contiguous():
        raise ValueError("corpus and corpus_offsets must be contiguous")
    if corpus_offsets.device != corpus.device:
        raise ValueError("corpus_offsets must be on the corpus's device")
    if int(seq_len) <= 0:
        raise ValueError("seq_len must be > 0")
    offs, n = _selection_args(corpus_offsets, index, perm, base, count)
    return corpus.reshape(-1), offs, n


def _device_plan_caps(n: int, corpus_elems: int, seq_len: int, max_rows, max_segs) -> tuple[int, int]:
    """Default capacities: ``pack_capacity`` of ``n`` sequences that hold at most the whole corpus (true of any
    selection without repeats; an index with repeats that carries more tokens than the corpus holds overflows
    them, which the plan reports as ``counts[0] = -1``: pass capacities of your own)."""
    cap_segs, cap_rows = pack_capacity(n, corpus_elems, seq_len)
    M = max(cap_segs, 1) if max_segs is None else int(max_segs)
    R = max(min(cap_rows, M), 1) if max_rows is None else int(max_rows)
    if M < 1 or R < 1:
        raise ValueError("max_segs and max_rows must be >= 1")
    if M >= (1 << 31) - 1:
        raise ValueError("max_segs does not fit the plan's int32 segment ids")
    return M, R


def _ref_selected(offs: torch.Tensor, n: int, index, perm, base) -> np.ndarray:
    return _ref_rows(offs.numel() - 1, n, index, perm, int(base)).numpy()


FFD_MAX_SEQS = 4096  # kFfdMaxSeqs (csrc/kernels/tokens_ffd.h): the bins of token_ffd_order's 64 x 64 tree


def check_ffd_count(n: int) -> None:
    if int(n) > FFD_MAX_SEQS:
        raise ValueError(f"the device first-fit-decreasing order takes at most {FFD_MAX_SEQS} sequences per batch, "
                         f"not {int(n)}: use the host plan (pack_order='ffd') for larger batches")


def ref_ffd_index(offsets, n: int, index=None, perm=None, base: int = 0, *, seq_len: int):
    """The definition of ``token_ffd_order``: ``(index int64 [n], ffd_rows, in_order_rows, used)`` for the ``n``
    selected sequences of the corpus with these ``offsets``. Lengths follow the batch descriptor (an index outside
    the corpus, or offsets that decrease, give an empty sequence); ``index`` is the selection in first-fit-decreasing
    order (``ffd_order_py``) when that packs rows of ``seq_len`` tokens into fewer rows than the given order does
    (``in_order_rows_py``), else the selection as given -- ``ffd_if_it_wins``, in NumPy, no native code."""
    from ..models.tokens import ffd_order_py, in_order_rows_py

    offs = offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)
    offs = offs.reshape(-1).astype(np.int64)
    if index is not None:
        q = index.to("cpu", torch.int64).numpy() if isinstance(index, torch.Tensor) else np.asarray(index, np.int64)
    else:
        q = _ref_rows(len(offs) - 1, int(n), None, perm, int(base)).numpy()
    q = q.reshape(-1)
    ok = (q >= 0) & (q < len(offs) - 1)
    qq = np.where(ok, q, 0)
    lens = np.where(ok, np.maximum(offs[qq + 1] - offs[qq], 0), 0) if len(offs) > 1 else np.zeros(len(q), np.int64)
    order, ffd_rows = ffd_order_py(lens, int(seq_len))
    in_order = in_order_rows_py(lens, int(seq_len))
    used = int(ffd_rows < in_order)
    return torch.from_numpy(q[order] if used else q.copy()), int(ffd_rows), int(in_order), used


def ffd_index_device(corpus_offsets: torch.Tensor, *, index: torch.Tensor | None = None,
                     perm: FeistelPermutation | None = None, base: int = 0, count: int | None = None, seq_len: int,
                     out: torch.Tensor | None = None, stream=None) -> dict:
    """The ``pack_order="ffd"`` rule of the token paths (``ffd_if_it_wins``) with nothing computed on the host: of the
    sequences selected as ``pack_tokens_indexed_device`` selects them (at most ``FFD_MAX_SEQS``), ``index`` = their
    corpus indices (int64 [n]) in first-fit-decreasing order when that order packs rows of ``seq_len`` tokens into
    fewer rows than the given one, else as given, and ``counts`` = int64 ``[ffd_rows, in_order_rows, used]``. One
    launch of one workgroup (``token_ffd_order``); no copy, no synchronisation. ``out``: an int64 device tensor of
    ``n + 3`` entries both are carved from. CPU tensors take the reference path (``ref_ffd_index``)."""
    if not isinstance(corpus_offsets, torch.Tensor) or corpus_offsets.dtype != torch.int64:
        raise TypeError("corpus_offsets must be an int64 tensor")
    if not corpus_offsets.is_contiguous():
        raise ValueError("corpus_offsets must be contiguous")
    if int(seq_len) <= 0:
        raise ValueError("seq_len must be > 0")
    offs, n = _selection_args(corpus_offsets, index, perm, base, count)
    check_ffd_count(n)
    if not offs.is_cuda:
        idx, ffd_rows, in_order, used = ref_ffd_index(offs, n, index, perm, base, seq_len=seq_len)
        return {"index": idx, "counts": torch.tensor([ffd_rows, in_order, used], dtype=torch.int64)}
    handle, stream = _stream_pair(stream, offs.device)
    if out is None:
        with torch.cuda.stream(stream):
            out = torch.empty(n + 3, dtype=torch.int64, device=offs.device)
    elif out.dtype != torch.int64 or out.device != offs.device or out.numel() < n + 3 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 tensor of {n + 3} entries on the offsets' device")
    out = out.view(-1)
    _native.hip().token_ffd_order(corpus_offsets=offs.data_ptr(), n_corpus=offs.numel() - 1, n=n, seq_len=int(seq_len),
                                  index_out=out.data_ptr(), counts=out.data_ptr() + 8 * n, stream=handle,
                                  **(_index_kw(index, perm, base) if n else _index_kw(None, None, 0)))
    return {"index": out[:n], "counts": out[n:n + 3]}


def pack_tokens_indexed_device(corpus: torch.Tensor, corpus_offsets: torch.Tensor, *,
                               index: torch.Tensor | None = None, perm: FeistelPermutation | None = None,
                               base: int = 0, count: int | None = None, seq_len: int, pad_id: int = 0,
                               position_dtype=torch.int64, max_rows: int | None = None, max_segs: int | None = None,
                               out: torch.Tensor | None = None, stream=None, labels: bool = False,
                               ignore_index: int = -100, pack_order: str = "in_order") -> dict:
    """``pack_tokens_indexed`` with nothing computed on the host: ``corpus`` (flat int32 / 16-bit ids) and
    ``corpus_offsets`` (int64 [n_corpus + 1]) are device tensors, and the sequences are selected as ``gather_rows``
    selects rows -- a device ``index``, or positions ``[base, base + count)`` of ``perm`` (evaluated inline by the
    kernel), or of the identity. Three launches, no copy and no synchronisation: ``token_batch_descriptor``
    (src_start, running offsets, each segment's corpus element), ``pack_plan_device`` (the in-order plan and its
    counts), and ``pad_pack_tokens_indexed`` reading the counts from device memory.

    Shapes are static: ``max_rows`` rows (rows past the plan's are padding: pad_id, mask 0, position 0, segment
    -1) and ``cu_seqlens`` of ``max_segs`` + 1 entries whose entries past ``n_seg`` equal the token count
    (zero-length trailing sequences). Returns ``input_ids``, ``attention_mask``, ``position_ids``, ``segment_ids``,
    ``cu_seqlens`` and ``counts`` = device int64 ``[n_rows, n_seg, n_tokens, max_seg]`` (``n_rows`` = -1 when a
    capacity was too small: every row is then padding and ``cu_seqlens`` is all zero). ``out``: a uint8 device
    buffer of ``device_plan_bytes(n, max_segs, max_rows) + device_batch_bytes(max_rows, seq_len, max_segs)``
    bytes that everything is carved from, else one allocation. ``labels=True`` adds ``labels`` (int64, the
    next-token labels of ``ref_token_labels``, written by the pack launch; all ``ignore_index`` for an overflowed
    plan) and both byte counts take ``labels=True``. CPU tensors take the reference path (``ref_gather_ragged`` +
    ``ref_pack_plan`` + ``ref_pack_tokens``): the same dict.

    ``pack_order="ffd"`` packs the selected sequences in the order of ``ffd_index_device`` (first-fit-decreasing
    when it needs fewer rows, at most ``FFD_MAX_SEQS`` sequences): one more launch, ``token_ffd_order``, in front of
    the three, which then run on its index; the plan window (``device_plan_bytes(..., ffd=True)``) also holds that
    index and its counts. The dict is the same. The CPU path applies ``ref_ffd_index`` first."""
    flat, offs, n = _device_plan_args(corpus, corpus_offsets, index, perm, base, count, seq_len, position_dtype)
    ignore_index = check_ignore_index(labels, ignore_index)
    if pack_order not in ("in_order", "ffd"):
        raise ValueError("pack_order must be 'in_order' or 'ffd'")
    ffd = pack_order == "ffd"
    if ffd:
        check_ffd_count(n)
    S = int(seq_len)
    M, R = _device_plan_caps(n, flat.numel(), S, max_rows, max_segs)
    if not flat.is_cuda:
        sel = _ref_selected(offs, n, index, perm, base)
        if ffd:
            sel = ref_ffd_index(offs, n, index, perm, base, seq_len=S)[0].numpy()
        tokens, dofs = ref_gather_ragged(flat, offs, sel)
        rs, re_, so = ref_pack_plan(dofs.numpy(), S)
        n_seg, n_tokens = len(so) - 1, int(dofs[-1])
        ok = n_seg <= M and len(rs) <= R
        keep = slice(None) if ok else slice(0, 0)
        ids, mask, pos, seg = ref_pack_tokens(tokens, rs[keep], re_[keep], so, S, pad_id, position_dtype, fill_rows=R)
        cu = torch.full((M + 1,), n_tokens if ok else 0, dtype=torch.int32)
        if ok:
            cu[:n_seg + 1] = torch.from_numpy(so.astype(np.int32))
        max_seg = int(np.diff(so).max()) if n_seg else 0
        counts = torch.tensor([len(rs) if ok else -1, n_seg, n_tokens, max_seg], dtype=torch.int64)
        r = {"input_ids": ids, "attention_mask": mask, "position_ids": pos, "segment_ids": seg, "cu_seqlens": cu,
             "counts": counts}
        if labels:
            r["labels"] = ref_token_labels(ids, mask, seg, ignore_index)
        return r
    plan_b = device_plan_bytes(n, M, R, ffd=ffd)
    handle, stream = _stream_pair(stream, flat.device)
    with torch.cuda.stream(stream):
        buf = _token_out_buffer(out, plan_b + device_batch_bytes(R, S, M, position_dtype, labels), flat.device)
    return launch_device_plan(
        buf.data_ptr(), buf[plan_b:], corpus_ptr=flat.data_ptr(), corpus_elems=flat.numel(),
        tok16=flat.dtype in _TOK16, corpus_offsets_ptr=offs.data_ptr(), n_corpus=offs.numel() - 1,
        selector=_index_kw(index, perm, base) if n else _index_kw(None, None, 0), n=n, seq_len=S, pad_id=pad_id,
        pack=True, max_segs=M, max_rows=R,
        position_dtype=position_dtype, stream=handle, labels=labels, ignore_index=ignore_index, ffd=ffd)


def pad_tokens_indexed_device(corpus: torch.Tensor, corpus_offsets: torch.Tensor, *,
                              index: torch.Tensor | None = None, perm: FeistelPermutation | None = None,
                              base: int = 0, count: int | None = None, seq_len: int, pad_id: int = 0,
                              position_dtype=torch.int64, out: torch.Tensor | None = None, stream=None,
                              labels: bool = False, ignore_index: int = -100) -> dict:
    """``pad_tokens_indexed`` with nothing computed on the host (see ``pack_tokens_indexed_device``): two
    launches, ``token_batch_descriptor`` and ``pad_pack_tokens_indexed``. Returns ``input_ids``,
    ``attention_mask``, ``position_ids`` ([n, seq_len]) and ``counts`` = device int64 ``[n, 0, n_tokens,
    max_seg]`` (``n_tokens``: the tokens of the selected sequences before truncation to ``seq_len``; ``max_seg``:
    the longest row). ``out``: ``device_plan_bytes(n) + device_batch_bytes(n, seq_len)`` bytes. ``labels=True``
    adds ``labels`` (``ref_token_labels``), as in ``pack_tokens_indexed_device``. CPU tensors take the reference
    path (``ref_gather_ragged`` + ``ref_pad_tokens``)."""
    flat, offs, n = _device_plan_args(corpus, corpus_offsets, index, perm, base, count, seq_len, position_dtype)
    ignore_index = check_ignore_index(labels, ignore_index)
    S = int(seq_len)
    if not flat.is_cuda:
        tokens, dofs = ref_gather_ragged(flat, offs, _ref_selected(offs, n, index, perm, base))
        ids, mask, pos = ref_pad_tokens(tokens, dofs, S, pad_id, position_dtype)
        lens = np.diff(dofs.numpy())
        counts = torch.tensor([n, 0, int(dofs[-1]), int(min(lens.max(), S)) if n else 0], dtype=torch.int64)
        r = {"input_ids": ids, "attention_mask": mask, "position_ids": pos, "counts": counts}
        if labels:
            r["labels"] = ref_token_labels(ids, mask, None, ignore_index)
        return r
    plan_b = device_plan_bytes(n)
    handle, stream = _stream_pair(stream, flat.device)
    with torch.cuda.stream(stream):
        buf = _token_out_buffer(out, plan_b + device_batch_bytes(n, S, None, position_dtype, labels), flat.device)
    return launch_device_plan(
        buf.data_ptr(), buf[plan_b:], corpus_ptr=flat.data_ptr(), corpus_elems=flat.numel(),
        tok16=flat.dtype in _TOK16, corpus_offsets_ptr=offs.data_ptr(), n_corpus=offs.numel() - 1,
        selector=_index_kw(index, perm, base) if n else _index_kw(None, None, 0), n=n, seq_len=S, pad_id=pad_id,
        pack=False,
        position_dtype=position_dtype, stream=handle, labels=labels, ignore_index=ignore_index)


# ------------------------------------- the token stream: full [B, S] rows cut from the epoch's documents
def _stream_order(n: int, perm) -> np.ndarray:
    pos = np.arange(n, dtype=np.int64)
    return pos if perm is None else np.asarray(perm(pos), dtype=np.int64)


def _stream_lengths(offs: np.ndarray, q: np.ndarray) -> np.ndarray:
    return np.maximum(offs[q + 1] - offs[q], 0) if q.size else np.zeros(0, dtype=np.int64)


def _host_order(order, perm) -> np.ndarray | None:
    """An ``order=`` argument as a flat int64 array on the host (None: not given)."""
    if order is None:
        return None
    if perm is not None:
        raise ValueError("give either order or perm, not both")
    q = order.detach().cpu().numpy() if isinstance(order, torch.Tensor) else np.asarray(order)
    if q.dtype != np.int64:
        raise TypeError("order must be int64")
    return np.ascontiguousarray(q.reshape(-1))


def _order_lengths(offs: np.ndarray, q: np.ndarray) -> np.ndarray:
    """Lengths of the documents of an explicit order; an id outside the corpus is an empty document, as in the
    kernels."""
    inside = (q >= 0) & (q < offs.size - 1)
    qc = np.where(inside, q, 0)
    return np.where(inside, _stream_lengths(offs, qc), 0) if q.size else np.zeros(0, dtype=np.int64)


def _stream_default_segs(n: int, rows: int, seq_len: int, shuffled_rows: bool = False) -> int:
    """A capacity that needs no length: every document that touches a window holds one of its tokens. Shuffled
    rows: every row may cut a document at either end, and a segment holds at least one token."""
    n, rows, seq_len = int(n), int(rows), int(seq_len)
    if shuffled_rows:
        return max(1, min(min(n, rows * seq_len) + 2 * rows, rows * seq_len))
    return max(1, min(n, rows * seq_len) + rows - 1)


def stream_max_segments(lengths, rows: int, seq_len: int, shuffled_rows: bool = False) -> int:
    """The most segments a ``rows x seq_len`` window of the token stream can hold, in any document order: with
    ``k`` = the largest count of smallest non-empty lengths whose sum is ``<= rows * seq_len``, at most ``k`` + 2
    documents touch a window (``k`` inside it, one cut at either end), and each of the ``rows`` - 1 interior row
    boundaries splits at most one of them: ``min(k + 2, n_nonempty) + rows - 1`` (at least 1).

    ``shuffled_rows``: the bound for ``rows`` distinct rows picked anywhere in the stream (``row_perm`` /
    ``row_index`` of ``ref_stream_tokens``): the documents lying wholly inside the selected rows are distinct and
    total at most ``rows * seq_len`` tokens, at most ``min(k, n_nonempty)`` of them, and every row has at most one
    document cut at either end: ``max(1, min(k, n_nonempty) + 2 * rows)``. It covers distinct rows only: with a
    row repeated in ``row_index`` its whole documents count once per occurrence, the caller sizes ``max_segs`` and
    an overflow is reported as ``n_rows`` = -1."""
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    lens = np.sort(lens[lens > 0])
    k = int(np.searchsorted(np.cumsum(lens), int(rows) * int(seq_len), side="right"))
    if shuffled_rows:
        return max(1, min(k, int(lens.size)) + 2 * int(rows))
    return max(1, min(k + 2, int(lens.size)) + int(rows) - 1)


def _stream_row_select(row_perm, row_index, row_base: int, rows: int) -> np.ndarray | None:
    """The stream rows ``rho_k`` of a batch selected by ``row_perm`` / ``row_index`` (None: contiguous rows)."""
    if row_perm is None and row_index is None:
        return None
    if row_perm is not None and row_index is not None:
        raise ValueError("give either row_perm or row_index, not both")
    if row_index is not None:
        if int(row_base) != 0:
            raise ValueError("row_index selects the batch's rows itself: row_base must be 0")
        rho = (row_index.detach().cpu().numpy() if isinstance(row_index, torch.Tensor) else np.asarray(row_index))
        if rho.dtype != np.int64:
            raise TypeError("row_index must be int64")
        rho = rho.reshape(-1)
        if rho.size != int(rows):
            raise ValueError(f"row_index holds {rho.size} entries for {int(rows)} rows")
        return rho
    if int(row_base) + int(rows) > row_perm.n:
        raise IndexError("row_perm positions out of range")
    return np.asarray(row_perm(np.arange(int(row_base), int(row_base) + int(rows), dtype=np.int64)), dtype=np.int64)


def ref_stream_tokens(corpus: torch.Tensor, corpus_offsets, *, perm=None, row_base: int, rows: int, seq_len: int,
                      pad_id: int = 0, position_dtype=torch.int64, max_segs: int | None = None, labels: bool = False,
                      ignore_index: int = -100, row_perm: FeistelPermutation | None = None, row_index=None,
                      order=None) -> dict:
    """The definition of the token stream format, in NumPy on the CPU (no plan code is involved)::

        stream = concat(corpus[offs[q_i] : offs[q_i + 1]] for i in range(n)),  q_i = perm(i) (or i),  T = len(stream)
        row r  = stream[(row_base + r) * S : (row_base + r + 1) * S]

    Documents carry their own EOS: nothing is inserted. Positions at or past ``T`` are padding (``pad_id``, mask
    0, position 0, segment -1). A segment is a maximal run of one document inside one row, numbered in row-major
    order across the batch (an empty document makes none); ``position_ids`` restart at 0 in every segment, also
    where a document continues from the previous row -- the rule the pack mode applies to the chunks of an
    over-long sequence. Returns ``input_ids``, ``attention_mask``, ``position_ids``, ``segment_ids`` ([rows, S]),
    ``cu_seqlens`` (int32 [max_segs + 1]: the batch-local segment starts, entries past ``n_seg`` = the batch's
    token count) and ``counts`` = int64 ``[n_rows, n_seg, n_tokens, max_seg]`` (``n_rows``: the rows holding a
    token); ``labels=True`` adds ``labels`` = ``ref_token_labels`` of the batch. ``n_seg > max_segs`` is an
    overflow: ``n_rows`` = -1, every row padding, ``cu_seqlens`` all zero, labels all ``ignore_index``.
    ``max_segs`` None: ``min(n, rows * S) + rows - 1``, which no window exceeds.

    Shuffled rows: with ``row_perm`` (a ``FeistelPermutation`` of the stream's ``T // S`` full rows) or ``row_index``
    (int64, ``rows`` entries, ``row_base`` 0; giving both is a ``ValueError``) batch row ``k`` is stream row
    ``rho_k = row_perm(row_base + k)`` or ``row_index[k]``::

        row k  = stream[rho_k * S : (rho_k + 1) * S]

    Segments keep their rule and are numbered row-major over the batch's rows in batch order; a row repeated in
    ``row_index`` makes its own segments at every occurrence. Only full rows can be selected: ``rho_k < 0`` or
    ``(rho_k + 1) * S > T`` (the partial last row and everything past it) makes the batch invalid, reported like
    an overflow (``n_rows`` = -1, every row padding, ``cu_seqlens`` all zero, labels all ``ignore_index``) with
    ``n_seg``, ``n_tokens`` and ``max_seg`` taken over the valid rows only; a valid batch has ``counts`` =
    ``[rows, n_seg, rows * S, max_seg]``. ``max_segs`` None: ``min(min(n, rows * S) + 2 * rows, rows * S)``.

    ``order`` (int64 array or tensor of corpus document ids, any length, repeats allowed; not together with
    ``perm``) gives the documents themselves: ``q_i = order[i]``, ``n = len(order)``. A segment belongs to a position
    of the order, not to a corpus id: two neighbouring copies of one document are two segments. An id outside the
    corpus is an empty document. This is how a ``TokenMix`` epoch is defined: ``order = ref_mix_order(...)``."""
    S, R, base = int(seq_len), int(rows), int(row_base)
    if S <= 0 or R < 1 or base < 0:
        raise ValueError("seq_len must be > 0, rows >= 1 and row_base >= 0")
    rho = _stream_row_select(row_perm, row_index, base, R)
    offs = torch.as_tensor(corpus_offsets).to("cpu", torch.int64).reshape(-1).numpy()
    q = _host_order(order, perm)
    if q is None:
        n = offs.size - 1
        q = _stream_order(n, perm)
        lens = _stream_lengths(offs, q)
    else:
        n = q.size
        lens = _order_lengths(offs, q)
    table = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lens, dtype=np.int64)])
    M = _stream_default_segs(n, R, S, rho is not None) if max_segs is None else int(max_segs)
    if rho is None:
        g = base * S + np.arange(R * S, dtype=np.int64)
        live = g < table[-1]  # the valid positions are a prefix of the batch
        rows_ok = True
    else:
        row_ok = (rho >= 0) & (rho < table[-1] // S)  # full rows only
        g = (np.where(row_ok, rho, 0)[:, None] * S + np.arange(S, dtype=np.int64)).reshape(-1)
        live = np.repeat(row_ok, S)
        rows_ok = bool(row_ok.all())
    at = np.flatnonzero(live)  # batch positions of the tokens; the counts of an invalid batch are the valid rows'
    n_tok = int(at.size)
    gv = g[at]
    d = np.searchsorted(table, gv, side="right") - 1  # the last document starting at or before g: never an empty one
    new = np.ones(n_tok, dtype=bool)
    new[1:] = (d[1:] != d[:-1]) | (gv[1:] % S == 0)
    starts = np.flatnonzero(new)
    n_seg = int(starts.size)
    seg = np.cumsum(new) - 1
    local = np.arange(n_tok, dtype=np.int64)
    ok = n_seg <= M and rows_ok
    ids = np.full(R * S, int(pad_id), dtype=np.int32)
    mask = np.zeros(R * S, dtype=np.uint8)
    pos = np.zeros(R * S, dtype=np.int64)
    sid = np.full(R * S, -1, dtype=np.int32)
    cu = np.zeros(M + 1, dtype=np.int32)
    if ok and n_tok:
        flat = widen_tokens(corpus.cpu().reshape(-1)).numpy()
        ids[at] = flat[offs[q[d]] + (gv - table[d])]
        mask[at] = 1
        pos[at] = local - starts[seg]
        sid[at] = seg
    if ok:
        cu[:n_seg] = at[starts]
        cu[n_seg:] = n_tok
    max_seg = int(np.diff(np.append(starts, n_tok)).max()) if n_seg else 0
    counts = torch.tensor([-(-n_tok // S) if ok else -1, n_seg, n_tok, max_seg], dtype=torch.int64)
    r = {"input_ids": torch.from_numpy(ids).view(R, S), "attention_mask": torch.from_numpy(mask).view(R, S),
         "position_ids": torch.from_numpy(pos).to(position_dtype).view(R, S),
         "segment_ids": torch.from_numpy(sid).view(R, S), "cu_seqlens": torch.from_numpy(cu), "counts": counts}
    if labels:
        r["labels"] = ref_token_labels(r["input_ids"], r["attention_mask"], r["segment_ids"], ignore_index)
    return r


def token_stream_table(corpus_offsets: torch.Tensor, perm: FeistelPermutation | None = None,
                       out: torch.Tensor | None = None, stream=None, scratch: torch.Tensor | None = None,
                       order=None):
    """``table`` (int64 [n + 1]) of the token stream of an epoch: ``table[i]`` = the tokens in front of document
    ``i`` of the order (``perm``, or the identity), ``table[n]`` = the stream's length. Device offsets: the
    ``token_stream_table`` kernels (a three-launch device-wide scan with the permutation evaluated inline: no
    n-sized index, no host step); ``out``: an int64 device tensor of n + 1 entries, ``scratch``: one of
    ``_native.hip().token_stream_table_scratch(n)``, else allocated here. CPU offsets: NumPy.

    ``order`` (not together with ``perm``): the table of an explicit order of corpus document ids (an int64 tensor
    on the offsets' device, or an array for CPU offsets), of any length ``n = len(order)``, repeats allowed."""
    if not isinstance(corpus_offsets, torch.Tensor) or corpus_offsets.dtype != torch.int64:
        raise TypeError("corpus_offsets must be an int64 tensor")
    offs = corpus_offsets.reshape(-1)
    if offs.numel() < 1 or not offs.is_contiguous():
        raise ValueError("corpus_offsets must be contiguous and hold at least one entry")
    n_corpus = n = offs.numel() - 1
    if perm is not None and perm.n != n:
        raise IndexError("the permutation's domain is not the corpus")
    if order is not None and perm is not None:
        raise ValueError("give either order or perm, not both")
    if not offs.is_cuda:
        o = offs.numpy()
        if order is not None:
            q = _host_order(order, None)
            n, lens = q.size, _order_lengths(o, q)
        else:
            lens = _stream_lengths(o, _stream_order(n, perm))
        t = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lens)])
        t = torch.from_numpy(t.astype(np.int64))
        if out is not None:
            out[:n + 1].copy_(t)
            return out[:n + 1]
        return t
    if order is not None:
        order = _device_order(order, offs.device)
        n = order.numel()
    h = _native.hip()
    handle, stream = _stream_pair(stream, offs.device)
    need = h.token_stream_table_scratch(n)
    with torch.cuda.stream(stream):
        if out is None:
            out = torch.empty(n + 1, dtype=torch.int64, device=offs.device)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.int64, device=offs.device)
    for name, t, size in (("out", out, n + 1), ("scratch", scratch, need)):
        if t.dtype != torch.int64 or t.device != offs.device or not t.is_contiguous() or t.numel() < size:
            raise ValueError(f"{name} must be a contiguous int64 tensor of >= {size} entries on the offsets' device")
    h.token_stream_table(corpus_offsets=offs.data_ptr(), n_corpus=n_corpus, n=n, table=out.data_ptr(),
                         tile_sums=scratch.data_ptr(), stream=handle,
                         **(_index_kw(order, perm, 0) if n else _index_kw(None, None, 0)))
    return out[:n + 1]


def _device_order(order, dev) -> torch.Tensor:
    """An ``order=`` argument of the GPU ops: a flat, contiguous int64 tensor on ``dev``."""
    if not isinstance(order, torch.Tensor) or order.dtype != torch.int64:
        raise TypeError("order must be an int64 tensor")
    if order.device != dev or not order.is_contiguous():
        raise ValueError("order must be a contiguous tensor on the corpus's device")
    return order.reshape(-1)


def token_stream_bytes(rows: int, seq_len: int, max_segs: int, position_dtype=torch.int64,
                       labels: bool = False, shuffled_rows: bool = False) -> tuple[int, int]:
    """(plan bytes, batch bytes) of one token stream batch. The plan -- seg_src [max_segs], seg_offsets
    [max_segs + 1], row_start / row_end [rows] -- lives between the two launches and nothing a caller holds is
    there; the batch is ``device_batch_bytes``: the outputs, ``cu_seqlens`` of capacity ``max_segs`` + 1 and the
    four int64 counts. ``shuffled_rows``: the plan of ``token_stream_plan_rows``, which keeps four more int64 per
    row between its two launches."""
    plan = _align16(8 * max_segs) + _align16(8 * (max_segs + 1)) + 2 * _align16(8 * rows)
    if shuffled_rows:
        plan += _align16(8 * 4 * rows)
    return plan, device_batch_bytes(rows, seq_len, max_segs, position_dtype, labels)


def _stream_plan_layout(plan_ptr: int, rows: int, max_segs: int) -> tuple[int, int, int, int, int]:
    """Addresses of seg_src, seg_offsets, row_start, row_end and (shuffled rows) the per-row scratch in a plan."""
    o_ss = plan_ptr
    o_so = o_ss + _align16(8 * max_segs)
    o_rs = o_so + _align16(8 * (max_segs + 1))
    o_re = o_rs + _align16(8 * rows)
    return o_ss, o_so, o_rs, o_re, o_re + _align16(8 * rows)


def _launch_stream_emit(h, whole: torch.Tensor, plan: tuple, *, corpus_ptr: int, corpus_elems: int, tok16: bool,
                        rows: int, seq_len: int, pad_id: int, max_segs: int, position_dtype, stream: int,
                        labels: bool, ignore_index: int, plan_fn, plan_kw: dict, staging_ptr: int = 0,
                        max_blocks: int = 0, fim: dict | None = None) -> dict:
    """``plan_fn(counts=..., **plan_kw)`` and ``pad_pack_tokens_indexed`` over the plan it wrote (pack mode, counts
    read from device memory), with everything returned carved from ``whole``. ``staging_ptr``: the zero-copy form
    (``launch_stream_plan_zerocopy``) -- ``gather_stream_pieces`` between the two copies the batch's tokens from the
    corpus into that window, which the emit launch then reads as its corpus. ``fim`` (``scratch_ptr``: ``rows *
    seq_len`` int32 of 16-byte aligned device memory, ``args``: ``TokenFIM.device_args`` of the epoch): the emit
    launch renders its ids there and writes no labels, and ``token_fim`` -- one more launch behind it -- writes the
    batch's ``input_ids`` and ``labels``, keyed by the plan's ``seg_src``."""
    S, R, M = int(seq_len), int(rows), int(max_segs)
    o_ss, o_so, o_rs, o_re, _ = plan
    o_keys = o_ss
    out_b = token_output_bytes(R, S, M, position_dtype, labels)
    ids, mask, pos, seg, cu, *lab = carve_token_outputs(whole, R, S, M, position_dtype, labels)
    counts = whole[out_b:out_b + 32].view(torch.int64)
    c_ptr = counts.data_ptr()
    plan_fn(counts=c_ptr, **plan_kw)
    if staging_ptr:
        h.gather_stream_pieces(dst=staging_ptr, src=corpus_ptr, corpus_elems=corpus_elems, seg_src=o_ss,
                               seg_offsets=o_so, counts=c_ptr, max_segs=M, rows=R, seq_len=S,
                               elem_bytes=2 if tok16 else 4, max_blocks=int(max_blocks), stream=stream)
        # piece s starts at window element seg_offsets[s]: the plan's seg_offsets are the window's seg_src. A label
        # is the next token of the same row and segment (ti_labels4): the emit reads nothing outside the window
        corpus_ptr, corpus_elems, o_ss = staging_ptr, R * S, o_so
    h.pad_pack_tokens_indexed(
        corpus=corpus_ptr, corpus_elems=corpus_elems, src_start=0, seg_src=o_ss, offsets=0, row_start=o_rs,
        row_end=o_re, seg_offsets=o_so, n_seg=0, out_tokens=fim["scratch_ptr"] if fim else ids.data_ptr(),
        attn_mask=mask.data_ptr(), position_ids=pos.data_ptr(), pos_is_i64=position_dtype == torch.int64,
        segment_ids=seg.data_ptr(), cu_seqlens_out=cu.data_ptr(), rows=0, seq_len=S, pad_id=pad_id, mode=1,
        stream=stream, fill_rows=R, tok16=tok16, dev_counts=c_ptr, cu_cap=M,
        labels=lab[0].data_ptr() if labels and not fim else 0, ignore_index=ignore_index)
    if fim:
        launch_fim(h, ids_ptr=fim["scratch_ptr"], seg=seg, pos=pos, cu_ptr=cu.data_ptr(), cap=M, seg_keys_ptr=o_keys,
                   counts_ptr=c_ptr, out_ptr=ids.data_ptr(), labels_ptr=lab[0].data_ptr() if labels else 0,
                   ignore_index=ignore_index, rows=R, seq_len=S, fim_args=fim["args"], stream=stream)
    r = {"input_ids": ids, "attention_mask": mask, "position_ids": pos, "segment_ids": seg, "cu_seqlens": cu,
         "counts": counts}
    if labels:
        r["labels"] = lab[0]
    return r


def launch_stream_plan(plan_ptr: int, whole: torch.Tensor, *, corpus_ptr: int, corpus_elems: int, tok16: bool,
                       corpus_offsets_ptr: int, n_corpus: int, table_ptr: int, selector: dict, row_base: int,
                       rows: int, seq_len: int, pad_id: int, max_segs: int, position_dtype=torch.int64,
                       stream: int = 0, labels: bool = False, ignore_index: int = -100,
                       n: int | None = None, staging_ptr: int = 0, max_blocks: int = 0,
                       fim: dict | None = None) -> dict:
    """The two launches of one token stream batch on raw stream ``stream``: ``token_stream_plan`` and
    ``pad_pack_tokens_indexed`` (pack mode, counts read from device memory). ``plan_ptr`` / ``whole``: the two
    sizes of ``token_stream_bytes``, 16-byte aligned device memory; ``selector``: the ``RowIndex`` of the epoch's
    order with base 0, the one ``table_ptr``'s table was built with; ``n``: the order's length where it is not the
    corpus's document count (an explicit order). Nothing here allocates, copies or synchronises. Returns the dict of
    ``stream_tokens_indexed_device``. ``staging_ptr`` / ``max_blocks``: ``launch_stream_plan_zerocopy``'s; ``fim``:
    ``_launch_stream_emit``'s, a third launch."""
    h = _native.hip()
    S, R, M = int(seq_len), int(rows), int(max_segs)
    ignore_index = check_ignore_index(labels, ignore_index)
    plan = _stream_plan_layout(plan_ptr, R, M)
    o_ss, o_so, o_rs, o_re, _ = plan
    plan_kw = dict(table=table_ptr, corpus_offsets=corpus_offsets_ptr, n_corpus=n_corpus,
                   n=n_corpus if n is None else int(n), row_base=int(row_base), rows=R, seq_len=S, max_segs=M,
                   seg_offsets=o_so, seg_src=o_ss, row_start=o_rs, row_end=o_re, stream=stream, **selector)
    return _launch_stream_emit(h, whole, plan, corpus_ptr=corpus_ptr, corpus_elems=corpus_elems, tok16=tok16, rows=R,
                               seq_len=S, pad_id=pad_id, max_segs=M, position_dtype=position_dtype, stream=stream,
                               labels=labels, ignore_index=ignore_index, plan_fn=h.token_stream_plan, plan_kw=plan_kw,
                               staging_ptr=staging_ptr, max_blocks=max_blocks, fim=fim)


def launch_stream_plan_rows(plan_ptr: int, whole: torch.Tensor, *, corpus_ptr: int, corpus_elems: int, tok16: bool,
                            corpus_offsets_ptr: int, n_corpus: int, table_ptr: int, selector: dict,
                            row_selector: dict, stream_rows: int, rows: int, seq_len: int, pad_id: int,
                            max_segs: int, position_dtype=torch.int64, stream: int = 0, labels: bool = False,
                            ignore_index: int = -100, n: int | None = None, staging_ptr: int = 0,
                            max_blocks: int = 0, fim: dict | None = None) -> dict:
    """``launch_stream_plan`` for rows picked anywhere in the stream: the two launches of ``token_stream_plan_rows``
    and ``pad_pack_tokens_indexed``, the call it is for contiguous rows. ``plan_ptr``: the plan size of
    ``token_stream_bytes(..., shuffled_rows=True)``; ``row_selector``: the ``RowIndex`` arguments that select the
    batch's rows (``_index_kw`` of a device ``row_index``, or of ``row_perm`` at the batch's first position);
    ``stream_rows``: the stream's full rows, ``T // seq_len``; ``n``: as for ``launch_stream_plan``. Nothing here
    allocates, copies or synchronises."""
    h = _native.hip()
    S, R, M = int(seq_len), int(rows), int(max_segs)
    ignore_index = check_ignore_index(labels, ignore_index)
    plan = _stream_plan_layout(plan_ptr, R, M)
    o_ss, o_so, o_rs, o_re, o_scr = plan
    plan_kw = dict(table=table_ptr, corpus_offsets=corpus_offsets_ptr, n_corpus=n_corpus,
                   n=n_corpus if n is None else int(n), stream_rows=int(stream_rows), rows=R, seq_len=S, max_segs=M,
                   seg_offsets=o_so, seg_src=o_ss, row_start=o_rs, row_end=o_re, scratch=o_scr, stream=stream,
                   **selector, **{"rows_" + k: v for k, v in row_selector.items()})
    return _launch_stream_emit(h, whole, plan, corpus_ptr=corpus_ptr, corpus_elems=corpus_elems, tok16=tok16, rows=R,
                               seq_len=S, pad_id=pad_id, max_segs=M, position_dtype=position_dtype, stream=stream,
                               labels=labels, ignore_index=ignore_index, plan_fn=h.token_stream_plan_rows,
                               plan_kw=plan_kw, staging_ptr=staging_ptr, max_blocks=max_blocks, fim=fim)


def stream_staging_bytes(rows: int, seq_len: int, token_bytes: int) -> int:
    """Bytes of the staging window of one zero-copy token stream batch: ``rows * seq_len`` ids of the corpus's
    width, what ``gather_stream_pieces`` writes and the emit launch reads."""
    return _align16(int(rows) * int(seq_len) * int(token_bytes))


def stream_zerocopy_window_bytes(rows: int, seq_len: int, max_segs: int, token_bytes: int,
                                 shuffled_rows: bool = False) -> int:
    """Bytes of a zero-copy stream batch's window between its launches: the plan of ``token_stream_bytes`` and,
    behind it, the staging window (``stream_staging_bytes``)."""
    plan, _ = token_stream_bytes(rows, seq_len, max_segs, shuffled_rows=shuffled_rows)
    return plan + stream_staging_bytes(rows, seq_len, token_bytes)


def launch_stream_plan_zerocopy(plan_ptr: int, whole: torch.Tensor, *, max_blocks: int = 0, **kw) -> dict:
    """``launch_stream_plan`` for a corpus the emit launch should not read token by token -- pinned, device-mapped
    host memory, where every load instruction is a PCIe read: ``token_stream_plan``, ``gather_stream_pieces`` (the
    batch's tokens, in 16-byte aligned loads, into a staging window in HBM; ``max_blocks`` > 0 caps its grid) and
    ``pad_pack_tokens_indexed`` out of that window, on one raw stream. ``plan_ptr``: device memory of
    ``stream_zerocopy_window_bytes`` bytes; ``corpus_ptr`` is the address the device reads the corpus at. The other
    arguments, the result and the promise -- nothing here allocates, copies or synchronises -- are
    ``launch_stream_plan``'s."""
    plan_b, _ = token_stream_bytes(kw["rows"], kw["seq_len"], kw["max_segs"])
    return launch_stream_plan(plan_ptr, whole, staging_ptr=plan_ptr + plan_b, max_blocks=max_blocks, **kw)


def launch_stream_plan_rows_zerocopy(plan_ptr: int, whole: torch.Tensor, *, max_blocks: int = 0, **kw) -> dict:
    """``launch_stream_plan_zerocopy`` for rows picked anywhere in the stream (``launch_stream_plan_rows``);
    ``plan_ptr``: ``stream_zerocopy_window_bytes(..., shuffled_rows=True)`` bytes."""
    plan_b, _ = token_stream_bytes(kw["rows"], kw["seq_len"], kw["max_segs"], shuffled_rows=True)
    return launch_stream_plan_rows(plan_ptr, whole, staging_ptr=plan_ptr + plan_b, max_blocks=max_blocks, **kw)


def _stream_pieces_args(src, seg_src, seg_offsets, counts, rows: int, seq_len: int):
    flat = (src.cpu if isinstance(src, HostRows) else src).reshape(-1)
    if flat.element_size() not in (2, 4):
        raise TypeError("gather_stream_pieces: 2- or 4-byte elements")
    for name, t in (("seg_src", seg_src), ("seg_offsets", seg_offsets), ("counts", counts)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_contiguous():
            raise TypeError(f"gather_stream_pieces: {name} must be a contiguous int64 tensor")
    M = int(seg_src.numel())
    if M < 1 or seg_offsets.numel() < M + 1 or counts.numel() < 2:
        raise ValueError("gather_stream_pieces: seg_src [max_segs >= 1], seg_offsets [max_segs + 1], counts [>= 2]")
    if int(rows) < 1 or int(seq_len) < 1 or int(rows) * int(seq_len) > 0x7FFFFFFF:
        raise ValueError("gather_stream_pieces: rows and seq_len must be >= 1 and rows * seq_len fit int32")
    return flat, M


def ref_gather_stream_pieces(src, seg_src, seg_offsets, counts, rows: int, seq_len: int,
                             out: torch.Tensor | None = None) -> torch.Tensor:
    """The definition of ``gather_stream_pieces``, in NumPy on the CPU: a copy of ``out`` (zeros without one) of
    ``rows * seq_len`` elements with ``out[g] = src[seg_src[s] + g - seg_offsets[s]]`` for ``seg_offsets[s] <= g <
    seg_offsets[s + 1]``, ``s < n_seg = counts[1]``, ``g < min(seg_offsets[n_seg], min(counts[0], rows) *
    seq_len)``. Nothing is written for ``counts[0] < 0``, ``n_seg`` = 0 or ``n_seg > len(seg_src)``, nor for a piece
    whose source range is not inside the source."""
    flat, M = _stream_pieces_args(src, seg_src, seg_offsets, counts, rows, seq_len)
    a = flat.cpu().numpy()
    ss, so, c = seg_src.cpu().numpy(), seg_offsets.cpu().numpy(), counts.cpu().numpy()
    n = int(rows) * int(seq_len)
    res = np.zeros(n, dtype=a.dtype) if out is None else out.detach().cpu().reshape(-1)[:n].numpy().copy()
    n_rows, n_seg = int(c[0]), int(c[1])
    if n_rows > 0 and 0 < n_seg <= M:
        limit = min(int(so[n_seg]), min(n_rows, int(rows)) * int(seq_len))
        for s in range(n_seg):
            lo, hi, e0 = int(so[s]), int(so[s + 1]), int(ss[s])
            if e0 < 0 or e0 + (hi - lo) > a.size:
                continue
            g1 = min(hi, limit)
            if g1 > lo:
                res[lo:g1] = a[e0:e0 + (g1 - lo)]
    return torch.from_numpy(res)


def gather_stream_pieces(src, seg_src: torch.Tensor, seg_offsets: torch.Tensor, counts: torch.Tensor, rows: int,
                         seq_len: int, *, out: torch.Tensor | None = None, max_blocks: int = 0,
                         stream=None) -> torch.Tensor:
    """The tokens of a token stream plan as one flat window (``ref_gather_stream_pieces``, the definition): ``src``
    is the corpus, a flat device tensor or ``HostRows`` (pinned, device-mapped host memory: every token of the batch
    crosses PCIe once, in 16-byte aligned loads) of 2- or 4-byte elements; ``seg_src`` [max_segs], ``seg_offsets``
    [max_segs + 1] and ``counts`` are the device arrays ``token_stream_plan`` / ``token_stream_plan_rows`` wrote. One
    launch of a static grid (the kernel reads the counts), no copy, no synchronisation; ``out``: ``rows * seq_len``
    elements of the source's dtype on the device, whose positions at or past the plan's tokens keep what they held
    (allocated here, uninitialised, without one). ``max_blocks`` > 0 caps the grid. CPU tensors take the
    reference."""
    if not _is_gpu(src):
        res = ref_gather_stream_pieces(src, seg_src, seg_offsets, counts, rows, seq_len, out)
        if out is not None:
            out.reshape(-1)[:res.numel()].copy_(res)
            return out.reshape(-1)[:res.numel()]
        return res
    flat, M = _stream_pieces_args(src, seg_src, seg_offsets, counts, rows, seq_len)
    if isinstance(src, torch.Tensor) and not src.is_contiguous():
        raise ValueError("gather_stream_pieces: source must be contiguous")
    n, dev = int(rows) * int(seq_len), seg_src.device
    for name, t in (("seg_src", seg_src), ("seg_offsets", seg_offsets), ("counts", counts)):
        if not t.is_cuda or t.device != dev or (isinstance(src, torch.Tensor) and t.device != src.device):
            raise ValueError(f"gather_stream_pieces: {name} must live on the source's GPU")
    handle, tstream = _stream_pair(stream, dev)
    if out is None:
        with torch.cuda.stream(tstream):
            out = torch.empty(n, dtype=flat.dtype, device=dev)
    elif not out.is_cuda or not out.is_contiguous() or out.dtype != flat.dtype or out.numel() < n:
        raise ValueError("gather_stream_pieces: bad out tensor")
    _native.hip().gather_stream_pieces(
        dst=out.data_ptr(), src=_src_addr(src), corpus_elems=flat.numel(), seg_src=seg_src.data_ptr(),
        seg_offsets=seg_offsets.data_ptr(), counts=counts.data_ptr(), max_segs=M, rows=int(rows),
        seq_len=int(seq_len), elem_bytes=flat.element_size(), max_blocks=int(max_blocks), stream=handle)
    return out.reshape(-1)[:n]


def stream_tokens_indexed_device(corpus: torch.Tensor, corpus_offsets: torch.Tensor, table: torch.Tensor | None = None,
                                 *, perm: FeistelPermutation | None = None, row_base: int, rows: int, seq_len: int,
                                 pad_id: int = 0, max_segs: int | None = None, position_dtype=torch.int64,
                                 labels: bool = False, ignore_index: int = -100, out: torch.Tensor | None = None,
                                 stream=None, row_perm: FeistelPermutation | None = None,
                                 row_index: torch.Tensor | None = None, stream_rows: int | None = None,
                                 order: torch.Tensor | None = None) -> dict:
    """Rows ``[row_base, row_base + rows)`` of the token stream (``ref_stream_tokens``, the definition) out of a
    corpus in HBM: ``corpus`` (flat int32 / 16-bit ids), ``corpus_offsets`` (int64 [n + 1]) and ``table``
    (``token_stream_table`` of the same ``perm``) are device tensors. Two launches -- ``token_stream_plan`` and
    ``pad_pack_tokens_indexed`` -- no copy, no synchronisation and no allocation beyond ``out``: a uint8 device
    buffer of ``sum(token_stream_bytes(rows, seq_len, max_segs, position_dtype, labels))`` bytes that the plan and
    everything returned are carved from, else one allocation. The result is static-shaped ([rows, seq_len],
    ``cu_seqlens`` of ``max_segs`` + 1 entries) and holds no padding except past the stream's end. ``max_segs``
    None: ``min(n, rows * seq_len) + rows - 1``, safe without a length (``stream_max_segments`` of the lengths is
    the tight one). CPU tensors take ``ref_stream_tokens`` (``table`` is not needed): the same dict.

    Shuffled rows (``ref_stream_tokens``): ``row_perm``, a ``FeistelPermutation`` of the stream's full rows, gives
    batch row ``k`` = stream row ``row_perm(row_base + k)``; ``row_index``, an int64 tensor of ``rows`` entries on
    the corpus's device (``row_base`` 0), gives stream row ``row_index[k]``. Either launches
    ``token_stream_plan_rows`` (two launches) in front of the same emit launch; ``out`` then holds
    ``sum(token_stream_bytes(..., shuffled_rows=True))`` bytes and ``max_segs`` None is ``min(min(n, rows * seq_len)
    + 2 * rows, rows * seq_len)``. ``stream_rows``: the stream's full rows ``T // seq_len``, the domain ``row_perm``
    must have; None with ``row_perm`` on the GPU reads ``table[n]`` back, the one synchronising step here.

    ``order`` (not together with ``perm``): an int64 tensor of corpus document ids on the corpus's device, of any
    length, repeats allowed (``token_mix_order`` writes one): the documents of the stream themselves, ``n =
    len(order)``, and ``table`` is ``token_stream_table(order=...)`` of it, ``n + 1`` entries."""
    flat, offs, _ = _device_plan_args(corpus, corpus_offsets, None, None, 0, 0, seq_len, position_dtype)
    ignore_index = check_ignore_index(labels, ignore_index)
    S, R, n_corpus = int(seq_len), int(rows), offs.numel() - 1
    if order is not None and perm is not None:
        raise ValueError("give either order or perm, not both")
    if order is not None:
        order = _device_order(order, flat.device) if flat.is_cuda else torch.from_numpy(_host_order(order, None))
    n = n_corpus if order is None else int(order.numel())
    if R < 1 or int(row_base) < 0:
        raise ValueError("rows must be >= 1 and row_base >= 0")
    if R * S > 0x7FFFFFFF:
        raise ValueError(f"{R} rows of {S} tokens overflow int32 cu_seqlens")
    if perm is not None and perm.n != n:
        raise IndexError("the permutation's domain is not the corpus")
    if row_perm is not None and row_index is not None:
        raise ValueError("give either row_perm or row_index, not both")
    by_rows = row_perm is not None or row_index is not None
    M = _stream_default_segs(n, R, S, by_rows) if max_segs is None else int(max_segs)
    if M < 1 or M >= (1 << 31) - 1:
        raise ValueError("max_segs must be >= 1 and fit the plan's int32 segment ids")
    if not flat.is_cuda:
        if row_perm is not None:
            o = offs.numpy()
            lens = np.maximum(np.diff(o), 0) if order is None else _order_lengths(o, order.numpy())
            _check_row_perm(row_perm, int(lens.sum()) // S if stream_rows is None else int(stream_rows), row_base, R)
        return ref_stream_tokens(flat, offs, perm=perm, row_base=row_base, rows=R, seq_len=S, pad_id=pad_id,
                                 position_dtype=position_dtype, max_segs=M, labels=labels, ignore_index=ignore_index,
                                 row_perm=row_perm, row_index=row_index, order=order)
    if (not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.device != flat.device
            or not table.is_contiguous() or table.numel() < n + 1):
        raise ValueError("table must be a contiguous int64 tensor of n + 1 entries on the corpus's device "
                         "(token_stream_table)")
    if row_index is not None:
        if not isinstance(row_index, torch.Tensor) or row_index.dtype != torch.int64:
            raise TypeError("row_index must be an int64 tensor")
        if row_index.device != flat.device or not row_index.is_contiguous() or row_index.numel() != R:
            raise ValueError(f"row_index must be a contiguous tensor of {R} entries on the corpus's device")
        if int(row_base) != 0:
            raise ValueError("row_index selects the batch's rows itself: row_base must be 0")
        row_selector = _index_kw(row_index.reshape(-1), None, 0)
    elif row_perm is not None:
        if stream_rows is None:
            stream_rows = int(table[n].item()) // S
        _check_row_perm(row_perm, int(stream_rows), row_base, R)
        row_selector = _index_kw(None, row_perm, int(row_base))
    plan_b, batch_b = token_stream_bytes(R, S, M, position_dtype, labels, by_rows)
    handle, stream = _stream_pair(stream, flat.device)
    with torch.cuda.stream(stream):
        buf = _token_out_buffer(out, plan_b + batch_b, flat.device)
    common = dict(corpus_ptr=flat.data_ptr(), corpus_elems=flat.numel(), tok16=flat.dtype in _TOK16,
                  corpus_offsets_ptr=offs.data_ptr(), n_corpus=n_corpus, n=n, table_ptr=table.data_ptr(),
                  selector=_index_kw(order, perm, 0) if n else _index_kw(None, None, 0), rows=R, seq_len=S,
                  pad_id=pad_id, max_segs=M, position_dtype=position_dtype, stream=handle, labels=labels,
                  ignore_index=ignore_index)
    if by_rows:
        return launch_stream_plan_rows(buf.data_ptr(), buf[plan_b:], row_selector=row_selector,
                                       stream_rows=0 if stream_rows is None else int(stream_rows), **common)
    return launch_stream_plan(buf.data_ptr(), buf[plan_b:], row_base=int(row_base), **common)


def ref_mix_order(mix, *, seed: int, epoch: int, shuffle: bool = True) -> np.ndarray:
    """The definition of a ``TokenMix`` epoch's document order, in NumPy: int64 ``[mix.n_order]`` corpus ids.

    With ``b`` = ``mix.bounds``, ``n_p``, ``full_p``, ``k_p`` and ``cbase`` as ``TokenMix`` defines them and ``N'`` =
    ``mix.n_order``::

        v = phi_e(i)                        phi_e = FeistelPermutation(N', seed, epoch), or the identity
        p: cbase[p] <= v < cbase[p + 1]     j = v - cbase[p]
        order[i] = b[p] + j % n_p                           if j < full_p * n_p      (the whole passes)
                 = b[p] + sigma_p(j - full_p * n_p)         otherwise                (the k_p extra documents)

    ``sigma_p = FeistelPermutation(n_p, part_seed_for(seed, p), 0)``, or the identity without ``shuffle``: it does
    not depend on the epoch, so a part's extra documents are the same set in every epoch and every epoch has the
    same token count."""
    n = int(mix.n_order)
    pos = np.arange(n, dtype=np.int64)
    v = np.asarray(FeistelPermutation(n, int(seed), int(epoch))(pos), dtype=np.int64) if shuffle else pos
    cbase = np.asarray(mix.cbase, dtype=np.int64)
    p = np.searchsorted(cbase[1:], v, side="right")  # the parts whose entries end at or before v
    j = v - cbase[p]
    n_docs = np.asarray(mix.n_docs, dtype=np.int64)
    span = np.asarray(mix.full, dtype=np.int64) * n_docs
    lo = np.asarray(mix.bounds[:-1], dtype=np.int64)
    whole = j < span[p]
    order = lo[p] + np.where(whole, j % n_docs[p], 0)
    for part in range(mix.parts):
        at = np.flatnonzero(~whole & (p == part))
        if at.size:
            r = j[at] - span[part]
            order[at] = lo[part] + (np.asarray(mix.inner_perm(seed, part)(r), dtype=np.int64) if shuffle else r)
    return order


def token_mix_order(mix, *, seed: int, epoch: int, shuffle: bool = True, device=None,
                    out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """``ref_mix_order`` as an int64 tensor on ``device`` (default: ``out``'s, else the CPU). On the GPU the
    ``token_mix_order`` kernel writes it: one launch, one thread per entry, the whole mix travelling as the kernel's
    argument, no copy and no synchronisation. ``out``: a contiguous int64 tensor of at least ``mix.n_order`` entries
    to write into (the result is its first ``n_order``), else allocated here."""
    n = int(mix.n_order)
    dev = out.device if out is not None else torch.device("cpu" if device is None else device)
    if out is not None and (out.dtype != torch.int64 or not out.is_contiguous() or out.numel() < n
                            or (device is not None and torch.device(device).type != dev.type)):
        raise ValueError(f"out must be a contiguous int64 tensor of >= {n} entries on the given device")
    if dev.type != "cuda":
        order = torch.from_numpy(ref_mix_order(mix, seed=seed, epoch=epoch, shuffle=shuffle))
        if out is None:
            return order
        out.reshape(-1)[:n].copy_(order)
        return out.reshape(-1)[:n]
    h = _native.hip()
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    handle, stream = _stream_pair(stream, dev)
    if out is None:
        with torch.cuda.stream(stream):
            out = torch.empty(n, dtype=torch.int64, device=dev)
    launch_mix_order(h, out.data_ptr(), mix.device_args(seed, shuffle), n_corpus=mix.n_documents, n=n,
                     perm=FeistelPermutation(n, int(seed), int(epoch)) if shuffle else None, stream=handle)
    return out.reshape(-1)[:n]


def launch_mix_order(h, order_ptr: int, parts: dict, *, n_corpus: int, n: int, perm, stream: int) -> None:
    """The one launch of ``token_mix_order`` on raw stream ``stream``: ``parts`` = ``TokenMix.device_args`` (it does
    not change with the epoch), ``perm`` = the epoch's permutation of the ``n`` entries or None."""
    h.token_mix_order(n_corpus=int(n_corpus), n=int(n), order=order_ptr, stream=stream, **parts,
                      **_index_kw(None, perm, 0))


# ------------------------------------------- fill-in-the-middle rearrangement of a rendered token batch
def _stream_seg_keys(corpus_offsets, batch: dict, *, perm=None, order=None, row_base: int, seq_len: int,
                        row_perm: FeistelPermutation | None = None, row_index=None) -> np.ndarray:
    """``seg_keys`` (int64 [n_seg]) of a ``ref_stream_tokens`` batch of the same arguments, as the stream plans write
    them (``seg_src``): the corpus element of each segment's first token. From the batch's own segments: segment
    ``s`` starts at batch position ``cu_seqlens[s]``, stream position ``g``, inside the order's document ``d``, at
    corpus element ``offs[q_d] + g - table[d]``. An overflowed or invalid batch has none."""
    S = int(seq_len)
    counts = batch["counts"].tolist()
    if counts[0] < 0:
        return np.zeros(0, dtype=np.int64)
    n_seg = int(counts[1])
    offs = torch.as_tensor(corpus_offsets).to("cpu", torch.int64).reshape(-1).numpy()
    q = _host_order(order, perm)
    if q is None:
        q = _stream_order(offs.size - 1, perm)
        lens = _stream_lengths(offs, q)
    else:
        lens = _order_lengths(offs, q)
    table = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lens, dtype=np.int64)])
    at = batch["cu_seqlens"].numpy()[:n_seg].astype(np.int64)
    rows = int(batch["input_ids"].shape[0])
    rho = _stream_row_select(row_perm, row_index, int(row_base), rows)
    k = at // S
    g = (int(row_base) + k if rho is None else rho[k]) * S + at % S
    d = np.searchsorted(table, g, side="right") - 1
    return offs[q[d]] + (g - table[d])


def _fim_n_rows(batch: dict):
    """The entry of a batch dict that holds ``n_rows`` (``counts`` of the ops, ``n_rows`` of the loaders), or None."""
    if "counts" in batch:
        return batch["counts"].reshape(-1)[:1]
    return batch.get("n_rows")


def _fim_check_batch(batch: dict, fim, labels: bool):
    from ..token_fim import TokenFIM

    if not isinstance(fim, TokenFIM):
        raise TypeError("fim must be a TokenFIM")
    for key in ("input_ids", "segment_ids", "position_ids", "cu_seqlens") + (("attention_mask",) if labels else ()):
        if not isinstance(batch.get(key), torch.Tensor):
            raise ValueError(f"fim_tokens: the batch has no tensor {key!r} (a batch of the pack or stream ops)")
    ids, seg, pos, cu = batch["input_ids"], batch["segment_ids"], batch["position_ids"], batch["cu_seqlens"]
    if ids.dtype != torch.int32 or ids.dim() != 2 or cu.dtype != torch.int32 or cu.dim() != 1 or cu.numel() < 1:
        raise TypeError("fim_tokens: input_ids must be int32 [R, S] and cu_seqlens int32 [capacity + 1]")
    for name, t in (("segment_ids", seg), ("position_ids", pos)):
        if t.dtype not in (torch.int32, torch.int64) or t.shape != ids.shape:
            raise TypeError(f"fim_tokens: {name} must be int32 or int64 of input_ids' shape")
    R, S = int(ids.shape[0]), int(ids.shape[1])
    if R < 1 or S < 1 or R * S > 0x7FFFFFFF:
        raise ValueError("fim_tokens: rows and seq_len must be >= 1 and rows * seq_len fit int32")
    return ids, seg, pos, cu, R, S


def ref_fim_tokens(batch: dict, fim, *, seg_keys, seed: int, epoch: int, labels: bool = False,
                   ignore_index: int = -100) -> dict:
    """The definition of the fill-in-the-middle rearrangement (``token_fim.TokenFIM`` has the arithmetic), in NumPy on
    the CPU. ``batch``: a dict of the pack or stream ops (``input_ids`` int32 [R, S], ``segment_ids``,
    ``position_ids``, ``cu_seqlens``; ``attention_mask`` for labels); ``seg_keys``: int64, the key of every segment
    (at least as many as the batch has segments; the loaders: the plan's ``seg_src``). A position belongs to segment
    ``s = segment_ids``, at offset ``j = position_ids`` of its ``L = cu_seqlens[s + 1] - cu_seqlens[s]`` tokens, which
    lie at columns ``[col - j, col - j + L)`` of its row; a position that is not part of such a segment (padding, ``s``
    outside the capacity or the keys, a run that leaves the row: none in a batch the ops rendered, given a key for
    every segment) keeps its token and has no target. Returns a new dict: ``input_ids`` is a new tensor, ``labels``
    (with ``labels=True``) are ``ref_token_labels`` of it -- labels of the input are dropped without --, every other
    entry is the input's. A batch with ``n_rows`` < 0 (``counts`` or ``n_rows`` of
    the dict: overflowed or invalid) is not rearranged."""
    ids_t, seg_t, pos_t, cu_t, R, S = _fim_check_batch(batch, fim, labels)
    ignore_index = check_ignore_index(labels, ignore_index)
    ids = ids_t.cpu().numpy()
    sid = seg_t.cpu().numpy().astype(np.int64)
    pos = pos_t.cpu().numpy().astype(np.int64)
    cu = cu_t.cpu().numpy().astype(np.int64)
    keys = (seg_keys.detach().cpu().numpy() if isinstance(seg_keys, torch.Tensor) else np.asarray(seg_keys))
    if keys.dtype != np.int64:
        raise TypeError("seg_keys must be int64")
    keys = keys.reshape(-1)
    cap = min(cu.size - 1, keys.size)
    n_rows = _fim_n_rows(batch)
    live = n_rows is None or int(torch.as_tensor(n_rows).reshape(-1)[0]) >= 0
    out = ids.copy()
    sound = (sid >= 0) & (sid < cap)
    if cap > 0:
        s = np.where(sound, sid, 0)
        L = cu[s + 1] - cu[s]
        col = np.broadcast_to(np.arange(S, dtype=np.int64), (R, S))
        row = np.broadcast_to(np.arange(R, dtype=np.int64)[:, None], (R, S))
        sound &= (pos >= 0) & (pos <= col)
        c0 = np.where(sound, col - pos, 0)  # the segment's first column
        sound &= (L >= 1) & (pos < L) & (c0 <= S - L)
    if live and sound.any():
        c0 = np.where(sound, c0, 0)
        L = np.where(sound, L, 1)
        tail = np.zeros((R, S), dtype=np.int64)
        if fim.eod_id is not None:
            tail = (ids[row, c0 + L - 1] == fim.eod_id).astype(np.int64)
        M = L - tail
        K = M - 3
        k4 = keys[s].astype(np.uint64) << np.uint64(2)
        ekey = np.uint64(fim.epoch_key(seed, epoch))
        u = [_mix64(ekey ^ _mix64(k4 + np.uint64(c))) for c in range(4)]
        sel = sound & (M >= fim.min_len) & ((u[0] >> np.uint64(40)) < np.uint64(fim.rate_q))
        spm = (u[1] >> np.uint64(40)) < np.uint64(fim.spm_q)
        K1 = np.where(sel, K + 1, 1).astype(np.uint64)
        x = (((u[2] >> np.uint64(32)) * K1) >> np.uint64(32)).astype(np.int64)
        y = (((u[3] >> np.uint64(32)) * K1) >> np.uint64(32)).astype(np.int64)
        a, b = np.minimum(x, y), np.maximum(x, y)
        n_suf = K - b
        j = pos
        PRE, SUF, MID = -1, -2, -3
        psm = np.select(
            [j == 0, j <= a, j == a + 1, j < a + 2 + n_suf, j == a + 2 + n_suf],
            [PRE, j - 1, SUF, b + (j - (a + 2)), MID], a + (j - (a + 3 + n_suf)))
        spm_src = np.select(
            [j == 0, j == 1, j < 2 + n_suf, j == 2 + n_suf],
            [PRE, SUF, b + (j - 2), MID], j - (3 + n_suf))
        src = np.where(spm, spm_src, psm)
        src = np.where(sel & (j < K + 3), src, j)  # untouched segments, and the EOD that stays last
        moved = sel & (src >= 0)
        gathered = ids[row, np.where(moved, c0 + src, 0)]
        out = np.where(moved, gathered, out)
        for code, tok in ((PRE, fim.prefix_id), (SUF, fim.suffix_id), (MID, fim.middle_id)):
            out = np.where(sel & (src == code), np.int32(tok), out)
        out = np.ascontiguousarray(out, dtype=np.int32)
    r = dict(batch)
    r.pop("labels", None)
    r["input_ids"] = torch.from_numpy(out)
    if labels:
        lab = ref_token_labels(r["input_ids"], batch["attention_mask"].cpu(), seg_t.cpu(), ignore_index)
        lab[torch.from_numpy(~sound)] = ignore_index  # a position outside every sound segment has no target
        r["labels"] = lab
    return r


def launch_fim(h, *, ids_ptr: int, seg: torch.Tensor, pos: torch.Tensor, cu_ptr: int, cap: int, seg_keys_ptr: int,
               counts_ptr: int, out_ptr: int, labels_ptr: int, ignore_index: int, rows: int, seq_len: int,
               fim_args: dict, stream: int) -> None:
    """The one launch of ``token_fim`` on raw stream ``stream``: ``fim_args`` = ``TokenFIM.device_args(seed, epoch)``;
    ``seg`` / ``pos`` give their addresses and widths. Nothing here allocates, copies or synchronises."""
    h.token_fim(ids=ids_ptr, seg=seg.data_ptr(), seg_is_i64=seg.dtype == torch.int64, pos=pos.data_ptr(),
                pos_is_i64=pos.dtype == torch.int64, cu=cu_ptr, cap=int(cap), seg_keys=seg_keys_ptr,
                counts=counts_ptr, out=out_ptr, labels=labels_ptr, ignore_index=int(ignore_index), rows=int(rows),
                seq_len=int(seq_len), stream=stream, **fim_args)


def fim_tokens(batch: dict, fim, *, seg_keys, seed: int, epoch: int, labels: bool = False,
               ignore_index: int = -100, stream=None) -> dict:
    """``ref_fim_tokens`` (the definition) of a batch on the device by the ``token_fim`` kernel: one launch, one
    workgroup per (row, 512 positions), no copy and no synchronisation; the new ``input_ids`` and ``labels`` are
    allocated here. The batch's tensors and ``seg_keys`` (an int64 tensor) must be contiguous and on one GPU; where
    the dict holds the device ``counts`` (or a device ``n_rows``) the kernel reads ``n_rows`` there. The label of a
    position is its segment's next rearranged token, which is ``ref_token_labels`` of the new ids for every batch
    the pack and stream ops render. A batch of CPU tensors takes the reference."""
    ids, seg, pos, cu, R, S = _fim_check_batch(batch, fim, labels)
    ignore_index = check_ignore_index(labels, ignore_index)
    if not ids.is_cuda:
        return ref_fim_tokens(batch, fim, seg_keys=seg_keys, seed=seed, epoch=epoch, labels=labels,
                              ignore_index=ignore_index)
    if not isinstance(seg_keys, torch.Tensor) or seg_keys.dtype != torch.int64:
        raise TypeError("fim_tokens: seg_keys must be an int64 tensor")
    n_rows = _fim_n_rows(batch)
    fim_args = fim.device_args(seed, epoch)
    if not isinstance(n_rows, torch.Tensor) or not n_rows.is_cuda:
        if n_rows is not None and int(torch.as_tensor(n_rows).reshape(-1)[0]) < 0:
            fim_args["rate_q"] = 0  # a host value the caller has read: an invalid batch is copied
        n_rows = None
    elif n_rows.dtype != torch.int64:
        raise TypeError("fim_tokens: counts / n_rows must be int64")
    dev = ids.device
    for name, t in (("input_ids", ids), ("segment_ids", seg), ("position_ids", pos), ("cu_seqlens", cu),
                    ("seg_keys", seg_keys), ("counts", n_rows)):
        if t is not None and (t.device != dev or not t.is_contiguous()):
            raise ValueError(f"fim_tokens: {name} must be contiguous and on the batch's GPU")
    handle, tstream = _stream_pair(stream, dev)
    with torch.cuda.stream(tstream):
        out = torch.empty((R, S), dtype=torch.int32, device=dev)
        lab = torch.empty((R, S), dtype=torch.int64, device=dev) if labels else None
    launch_fim(_native.hip(), ids_ptr=ids.data_ptr(), seg=seg, pos=pos, cu_ptr=cu.data_ptr(),
               cap=min(cu.numel() - 1, seg_keys.numel()), seg_keys_ptr=seg_keys.data_ptr(),
               counts_ptr=0 if n_rows is None else n_rows.data_ptr(), out_ptr=out.data_ptr(),
               labels_ptr=lab.data_ptr() if labels else 0, ignore_index=ignore_index, rows=R, seq_len=S,
               fim_args=fim_args, stream=handle)
    r = dict(batch)
    r.pop("labels", None)
    r["input_ids"] = out
    if labels:
        r["labels"] = lab
    return r


def _check_row_perm(row_perm: FeistelPermutation, stream_rows: int, row_base: int, rows: int) -> None:
    if row_perm.n != stream_rows:
        raise IndexError(f"row_perm permutes {row_perm.n} rows, the stream has {stream_rows} full rows")
    if int(row_base) + int(rows) > row_perm.n:
        raise IndexError("row_perm positions out of range")


# ----------------------------------------------------------------- reductions
def ref_checksum(x: torch.Tensor) -> int:
    b = x.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
    n = b.size // 4 * 4
    return int(b[:n].view(np.uint32).astype(np.uint64).sum()) & ((1 << 64) - 1)


def checksum(x: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Sum of the 32-bit words of ``x`` (u64 wrap-around) as a 1-element int64 tensor (accumulates into ``out``)."""
    if not x.is_contiguous():
        raise ValueError("checksum needs a contiguous tensor")
    nbytes = x.numel() * x.element_size()
    if not x.is_cuda:
        v = ref_checksum(x)
        v = v - (1 << 64) if v >= (1 << 63) else v
        res = torch.tensor([v], dtype=torch.int64)
        if out is not None:
            out += res
            return out
        return res
    if out is None:
        out = torch.zeros(1, dtype=torch.int64, device=x.device)
    h = _native.hip()
    scratch = torch.empty(h.CHECKSUM_MAX_BLOCKS, dtype=torch.int64, device=x.device)
    h.checksum_words(ptr=x.data_ptr(), bytes=nbytes - nbytes % 4, out=out.data_ptr(), scratch=scratch.data_ptr(),
                     scratch_len=scratch.numel(), stream=_stream_handle(stream))
    return out


class ChecksumAccumulator:
    """Running checksum of many tensors: one streaming launch per ``add``.

    Each of ``n_partials`` workgroups adds its share of every tensor into its own
    64-bit slot (single writer, stream-ordered, no atomics); ``value()`` reduces
    the slots. Same sum as ``checksum`` (u64 wrap-around of the 32-bit words).
    Launches on one accumulator must be ordered on one stream.
    """

    def __init__(self, device, n_partials: int = 1024):
        self.device = torch.device(device)
        self.n = int(n_partials)
        self.partials = torch.zeros(self.n, dtype=torch.int64, device=self.device) if self.device.type == "cuda" \
            else None
        self._cpu = 0

    def add(self, x: torch.Tensor, stream=None) -> None:
        if not x.is_contiguous():
            raise ValueError("checksum needs a contiguous tensor")
        nbytes = x.numel() * x.element_size()
        if self.partials is None or not x.is_cuda:
            self._cpu = (self._cpu + ref_checksum(x)) & ((1 << 64) - 1)
            return
        if x.device != self.device:
            raise ValueError(f"tensor on {x.device}, accumulator on {self.device}")
        _native.hip().checksum_accumulate(ptr=x.data_ptr(), bytes=nbytes - nbytes % 4,
                                          partials=self.partials.data_ptr(), n_partials=self.n,
                                          stream=_stream_handle(stream))

    def value(self, stream=None) -> int:
        """Sum so far as an unsigned 64-bit int (synchronises with the accumulating stream)."""
        tot = self._cpu
        if self.partials is not None:
            out = torch.zeros(1, dtype=torch.int64, device=self.device)
            _native.hip().checksum_finalize(partials=self.partials.data_ptr(), n_partials=self.n,
                                            out=out.data_ptr(), stream=_stream_handle(stream))
            tot += int(out.item())
        return tot & ((1 << 64) - 1)


def column_affine(stats: dict, mode: str = "standard", area_weighted: bool = False) -> tuple[list, list]:
    """(scale, bias) per column so that x*scale + bias normalises like the reference harness.

    ``standard``: (x - mean) / std. ``minmax``: (x - (max+min)/2) / ((max-min)/2).
    ``area_weighted`` keeps the last column un-centred and scales it by its mean
    (reference tests/run_ddl.py:45-77).
    """
    mean, std, mn, mx = (stats[k].double().cpu() for k in ("mean", "std", "min", "max"))
    if mode == "standard":
        centre, spread = mean.clone(), std.clone()
    elif mode == "minmax":
        centre, spread = 0.5 * (mx + mn), 0.5 * (mx - mn)
    else:
        raise ValueError("mode must be 'standard' or 'minmax'")
    if area_weighted:
        centre[-1], spread[-1] = 0.0, mean[-1]
    spread = torch.where(spread == 0, torch.ones_like(spread), spread)
    return (1.0 / spread).tolist(), (-centre / spread).tolist()


def normalize_columns(x: torch.Tensor, mode: str = "standard", out_dtype=None, stats: dict | None = None,
                      area_weighted: bool = False, stream=None) -> torch.Tensor:
    """Per-column normalisation of an [N, C<=16] f32 table on the device (column_stats + fused affine gather)."""
    if x.dim() != 2 or x.shape[1] > 16:
        raise ValueError("normalize_columns expects [N, C] with C <= 16")
    stats = stats or column_stats(x, stream=stream)
    sc, bi = column_affine(stats, mode, area_weighted)
    return gather_rows(x, out_dtype=out_dtype or torch.float32, scale=sc, bias=bi, plane=1, stream=stream)


def column_stats(x: torch.Tensor, stream=None) -> dict[str, torch.Tensor]:
    """Per-column sum / sumsq / min / max / mean / std (population) of an [N, C] f32 matrix, as float32 tensors.

    The sums and sums of squares are accumulated in float64 (on the GPU by the kernels, from the first add on),
    and ``mean = sum/n`` and ``std = sqrt(sumsq/n - mean^2)`` are formed from them in float64 before the one
    rounding to float32: a column whose mean is 1e3 or 1e4 times its spread keeps its std, which a float32
    ``sumsq/n - mean^2`` loses. ``sum`` and ``sumsq`` are the float64 totals rounded to float32; ``min`` and
    ``max`` are exact."""
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError("column_stats expects [N, C] float32")
    n, c = x.shape
    if not x.is_cuda:
        xd = x.double()
        acc = torch.zeros((4, c), dtype=torch.float64)
        acc[0], acc[1] = xd.sum(0), (xd * xd).sum(0)
        mn, mx = x.min(0).values, x.max(0).values
    else:
        x = x.contiguous()
        buf = _column_stats_init(c, x.device).clone()  # one launch sets up every accumulator
        acc = buf[:8 * c].view(torch.float64).view(4, c)  # sum, sumsq, and room for mean, std
        mn, mx = buf[8 * c:9 * c], buf[9 * c:]
        base = buf.data_ptr()
        _native.hip().column_stats(src=x.data_ptr(), n=n, cols=c, sum=base, sumsq=base + 8 * c, min=base + 32 * c,
                                   max=base + 36 * c, stream=_stream_handle(stream))
    torch.div(acc[:2], n, out=acc[2:])  # float64 mean and mean of squares
    torch.addcmul(acc[3], acc[2], acc[2], value=-1, out=acc[3]).clamp_min_(0).sqrt_()
    s, q, mean, std = acc.float().unbind(0)
    return {"sum": s, "sumsq": q, "min": mn, "max": mx, "mean": mean, "std": std}


@functools.lru_cache(maxsize=64)
def _column_stats_init(c: int, device: torch.device) -> torch.Tensor:
    """The start state of ``column_stats``'s accumulators for ``c`` columns, as one float32 buffer: 8c zeros (a
    float64 [4, c]), c times +inf (min), c times -inf (max). Built on the host, so that it is complete on the
    device whichever stream clones it first."""
    t = torch.zeros(10 * c, dtype=torch.float32)
    t[8 * c:9 * c], t[9 * c:] = float("inf"), float("-inf")
    return t.to(device)
