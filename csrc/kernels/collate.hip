// Collate kernels.
//
// collate_hwc_to_chw: decoded images usually arrive pixel-interleaved (HWC,
// uint8); models want planar NCHW bf16, normalised per channel. The kernel
// stages a 2048-pixel tile in LDS with coalesced 16 B loads, then every lane
// de-interleaves 8 consecutive pixels and writes one 16 B bf16 vector per
// channel plane -- both the global read and the global write are fully
// vectorised and coalesced; LDS absorbs the stride-C shuffle.
//
// split_columns: the reference hands the consumer a tuple of strided views of
// one [B, nValues] row block (ddl/mpi_dataloader.py:193-196). For device
// batches we emit the column groups as contiguous tensors in one pass fused
// with the permutation gather and the dtype cast.
#include "elem.h"
#include "launch.h"

namespace ddl {
namespace {

constexpr int kPix = 2048;  // pixels per tile: 8 per lane
// Dynamic LDS a launch may ask for without raising the kernel's limit through a function attribute.
constexpr size_t kPlainLdsBytes = 64 * 1024;

// grid: (tiles_per_image * batch); LDS: tile_px * C * sizeof(Tin) bytes. tile_px is kPix, or a smaller
// multiple of 8 for wide pixels (launch_hwc); lanes past the tile's pixels only help to stage it.
template <typename Tin, typename Tout>
__global__ void __launch_bounds__(kThreads) hwc_to_chw_kernel(Tout* __restrict__ dst, const Tin* __restrict__ src,
                                                              int64_t pixels, int32_t channels, int64_t tiles,
                                                              int32_t tile_px, RowIndex ri, Affine aff) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  Tin* tile = reinterpret_cast<Tin*>(lds_raw);
  const auto [img, t] = row_chunk(blockIdx.x, tiles);  // grid < 2^32 blocks
  const int64_t p0 = t * tile_px;
  const int npx = static_cast<int>(pixels - p0 < tile_px ? pixels - p0 : tile_px);
  const int64_t srow = source_row(ri, img);
  const Tin* s = src + (srow * pixels + p0) * channels;
  const int elems = npx * channels;
  const int bytes = elems * static_cast<int>(sizeof(Tin));
  // Stage: 16 B per lane when the span is 16 B aligned, element-wise otherwise.
  if ((reinterpret_cast<uintptr_t>(s) & 15u) == 0 && (bytes & 15) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    uint4* l4 = reinterpret_cast<uint4*>(tile);
    for (int i = threadIdx.x; i < bytes / 16; i += kThreads) l4[i] = s4[i];
  } else {
    for (int i = threadIdx.x; i < elems; i += kThreads) tile[i] = s[i];
  }
  __syncthreads();
  const int px = threadIdx.x * 8;
  const int64_t out_img = img * channels * pixels;
  for (int c = 0; c < channels; ++c) {
    const float sc = aff.enabled ? aff.scale[c] : 1.f;
    const float bi = aff.enabled ? aff.bias[c] : 0.f;
    const int64_t obase = out_img + c * pixels + p0;
    if (px + 8 <= npx && ((obase + px) & 7) == 0) {
      float f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = fmaf(Elem<Tin>::load1(tile + ((px + k) * channels + c)), sc, bi);
      Elem<Tout>::template store<8>(dst + (obase + px), f);
    } else {
      for (int k = 0; k < 8 && px + k < npx; ++k)
        Elem<Tout>::store1(dst + (obase + px + k), fmaf(Elem<Tin>::load1(tile + ((px + k) * channels + c)), sc, bi));
    }
  }
}

// Specialisation for the common case (uint8 RGB). Each workgroup stages a
// 4096-pixel (12 KB) tile: the kernel is bound by bytes in flight per CU
// (HBM latency x bandwidth is ~50 KB per CU), and 8 resident workgroups x 12 KB
// of loads cover it where 6 KB tiles did not (measured 77% -> see
// docs/PERFORMANCE.md). Each lane owns two 8-pixel groups; for each it pulls
// its 24 B out of LDS with three conflict-free ds_read_b64 (lane stride 24 B ->
// dword stride 6: the 32 lanes of a half-wave cover all 64 banks once) and
// de-interleaves in registers.
constexpr int kPix3 = 4096;

template <typename Tout>
__global__ void __launch_bounds__(kThreads) hwc3_u8_to_chw_kernel(Tout* __restrict__ dst, const uint8_t* __restrict__ src,
                                                                  int64_t pixels, int64_t tiles, RowIndex ri,
                                                                  Affine aff) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kPix3 * 3];
  const auto [img, t] = row_chunk(blockIdx.x, tiles);  // grid < 2^32 blocks
  const int64_t p0 = t * kPix3;
  const int npx = static_cast<int>(pixels - p0 < kPix3 ? pixels - p0 : kPix3);
  const uint8_t* s = src + (source_row(ri, img) * pixels + p0) * 3;
  const int bytes = npx * 3;
  if ((reinterpret_cast<uintptr_t>(s) & 15u) == 0 && (bytes & 15) == 0) {
    static_assert(kPix3 * 3 / 16 == 3 * kThreads, "three 16 B loads per lane");
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    uint4* l4 = reinterpret_cast<uint4*>(tile);
    const int n16 = bytes / 16;
    const int i0 = threadIdx.x, i1 = i0 + kThreads, i2 = i1 + kThreads;
    uint4 v0{}, v1{}, v2{};  // all loads issued before the first LDS write
    if (i0 < n16) v0 = s4[i0];
    if (i1 < n16) v1 = s4[i1];
    if (i2 < n16) v2 = s4[i2];
    if (i0 < n16) l4[i0] = v0;
    if (i1 < n16) l4[i1] = v1;
    if (i2 < n16) l4[i2] = v2;
  } else {
    for (int i = threadIdx.x; i < bytes; i += kThreads) tile[i] = s[i];
  }
  __syncthreads();
  const int64_t out_img = img * 3 * pixels;
#pragma unroll
  for (int g = 0; g < kPix3 / (kThreads * 8); ++g) {
    const int px = (g * kThreads + static_cast<int>(threadIdx.x)) * 8;
    if (px + 8 <= npx) {
      const uint64_t* l8 = reinterpret_cast<const uint64_t*>(tile + px * 3);
      const uint64_t w[3] = {l8[0], l8[1], l8[2]};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float sc = aff.enabled ? aff.scale[c] : 1.f;
        const float bi = aff.enabled ? aff.bias[c] : 0.f;
        float f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int b = 3 * k + c;  // byte index inside the lane's 24 bytes
          f[k] = fmaf(static_cast<float>((w[b >> 3] >> (8 * (b & 7))) & 0xffu), sc, bi);
        }
        const int64_t o = out_img + c * pixels + p0 + px;
        if ((o & 7) == 0) {
          Elem<Tout>::template store<8>(dst + o, f);
        } else {
          for (int k = 0; k < 8; ++k) Elem<Tout>::store1(dst + (o + k), f[k]);
        }
      }
    } else if (px < npx) {
      for (int c = 0; c < 3; ++c) {
        const float sc = aff.enabled ? aff.scale[c] : 1.f;
        const float bi = aff.enabled ? aff.bias[c] : 0.f;
        for (int k = 0; k < 8 && px + k < npx; ++k)
          Elem<Tout>::store1(dst + (out_img + c * pixels + p0 + px + k),
                             fmaf(static_cast<float>(tile[(px + k) * 3 + c]), sc, bi));
      }
    }
  }
}

// LDS bytes one workgroup of the generic kernel may request on the current device: the device's limit per
// workgroup, and no more than a launch gets without a function attribute. 0: the query failed.
size_t hwc_lds_limit() {
  int dev = 0, per_block = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || per_block <= 0)
    return 0;
  return static_cast<size_t>(per_block) < kPlainLdsBytes ? static_cast<size_t>(per_block) : kPlainLdsBytes;
}

template <typename Tin, typename Tout>
int launch_hwc(void* dst, const void* src, int64_t batch, int64_t pixels, int32_t channels, const RowIndex& ri,
               const Affine& aff, hipStream_t st) {
  if constexpr (std::is_same_v<Tin, uint8_t>) {
    if (channels == 3) {
      const int64_t tiles3 = (pixels + kPix3 - 1) / kPix3;
      if (batch * tiles3 >= (int64_t{1} << 32)) return -4;  // as below: one block per (image, tile)
      hipLaunchKernelGGL(hwc3_u8_to_chw_kernel<Tout>, dim3(static_cast<uint32_t>(batch * tiles3)), dim3(kThreads), 0,
                         st, static_cast<Tout*>(dst), static_cast<const uint8_t*>(src), pixels, tiles3, ri, aff);
      return static_cast<int>(hipGetLastError());
    }
  }
  // The tile is kPix pixels while that fits the LDS a workgroup may have (u8 and bf16 at every channel count,
  // f32 up to 8 channels); wider pixels halve it (f32 x 16 channels: 512 pixels), so the request never
  // passes the limit and no shape fails at launch.
  const size_t px_bytes = static_cast<size_t>(channels) * sizeof(Tin);
  const size_t limit = hwc_lds_limit();
  int32_t tile_px = kPix;
  while (tile_px > 8 && tile_px * px_bytes > limit) tile_px >>= 1;
  if (tile_px * px_bytes > limit) return -5;  // not even 8 pixels fit (or no limit could be read)
  const size_t lds = tile_px * px_bytes;
  const int64_t tiles = (pixels + tile_px - 1) / tile_px;
  if (batch * tiles >= (int64_t{1} << 32)) return -4;  // the grid is one block per (image, tile)
  hipLaunchKernelGGL((hwc_to_chw_kernel<Tin, Tout>), dim3(static_cast<uint32_t>(batch * tiles)), dim3(kThreads), lds,
                     st, static_cast<Tout*>(dst), static_cast<const Tin*>(src), pixels, channels, tiles, tile_px, ri,
                     aff);
  return static_cast<int>(hipGetLastError());
}

// ------------------------------------------------------------------ split ---
// Row tiles of one wavefront: rows are short (the reference's CI rows are 9
// floats), so a lane per (row, column) element would evaluate the row's
// Feistel permutation once per element -- 9x the 64-bit hash work per row,
// which made these kernels ALU-bound at ~0.2 TB/s. Instead each wave owns R
// (<= 64, tile_rows) consecutive output rows, lane l computes source_row() of
// row l of the tile ONCE, and the tile's rows*n_values elements are walked lane-contiguously
// (coalesced reads of each source row, coalesced per-group writes) with the
// source row fetched from its owner lane by a cross-lane shuffle. The shuffle
// is executed by all 64 lanes every iteration (uniform loop), so it never
// reads from a lane that has left the loop.
// Rows per wave tile. The Feistel cycle walk diverges: a wave runs until its slowest lane's row is
// placed (~10 rounds for 64 rows at the pointwise shape's n / 2^(2h) = 0.38), so the total ALU work
// is lowest with 64-row tiles. A small launch (one 4096-row batch = 64 such waves) is instead
// latency-bound on that chain: there the tile shrinks (down to 8 rows) until ~512 waves share it.
__host__ __device__ __forceinline__ int64_t tile_rows(int64_t n_rows) {
  int64_t r = 64;
  while (r > 8 && n_rows / r < 512) r >>= 1;
  return r;
}

template <typename F>
__device__ __forceinline__ void for_row_tiles(int64_t n_rows, int64_t n_values, const RowIndex& ri, F&& f) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = static_cast<int64_t>(gridDim.x) * (kThreads / 64);
  const int64_t R = tile_rows(n_rows);
  const int64_t n_tiles = (n_rows + R - 1) / R;
  const uint32_t nv = static_cast<uint32_t>(n_values);
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); t < n_tiles;
       t += waves) {
    const int64_t r0 = t * R;
    const int64_t rows = n_rows - r0 < R ? n_rows - r0 : R;
    const int64_t mine = lane < rows ? source_row(ri, r0 + lane) : 0;
    const uint32_t total = static_cast<uint32_t>(rows) * nv;  // <= 64 * n_values
    for (uint32_t base = 0; base < total; base += 64) {
      const uint32_t e = base + static_cast<uint32_t>(lane);
      const uint32_t rr = e < total ? e / nv : 0;
      const int64_t src_row = __shfl(mine, static_cast<int>(rr), 64);
      if (e < total) f(r0 + rr, static_cast<int>(e - rr * nv), src_row);
    }
  }
}

// Long rows (n_values > kTileMaxValues): a wave per (row, chunk of kRowChunk elements); the row's source
// is evaluated once per chunk (the same value in every lane) instead of once per element.
constexpr int64_t kTileMaxValues = 256;
constexpr int64_t kRowChunk = 4096;

template <typename F>
__device__ __forceinline__ void for_row_chunks(int64_t n_rows, int64_t n_values, const RowIndex& ri, F&& f) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = static_cast<int64_t>(gridDim.x) * (kThreads / 64);
  const int64_t chunks = (n_values + kRowChunk - 1) / kRowChunk;
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
       item < n_rows * chunks; item += waves) {
    const int64_t row = item / chunks;
    const int64_t c0 = (item - row * chunks) * kRowChunk;
    const int64_t c1 = c0 + kRowChunk < n_values ? c0 + kRowChunk : n_values;
    const int64_t src_row = source_row(ri, row);
    for (int64_t c = c0 + lane; c < c1; c += 64) f(row, static_cast<int>(c), src_row);
  }
}

template <typename F>
__device__ __forceinline__ void for_rows(int64_t n_rows, int64_t n_values, const RowIndex& ri, F&& f) {
  if (n_values <= kTileMaxValues)
    for_row_tiles(n_rows, n_values, ri, f);
  else
    for_row_chunks(n_rows, n_values, ri, f);
}

// waves the row walk of (n_rows, n_values) can use
inline int64_t row_walk_waves(int64_t n_rows, int64_t n_values) {
  return n_values <= kTileMaxValues ? (n_rows + tile_rows(n_rows) - 1) / tile_rows(n_rows)
                                    : n_rows * ((n_values + kRowChunk - 1) / kRowChunk);
}

__device__ __forceinline__ int group_of(const SplitSpec& spec, int* col) {
  int g = 0;
  while (g < spec.n_groups - 1 && *col >= spec.width[g]) {
    *col -= spec.width[g];
    ++g;
  }
  return g;
}

// output element of group g, row `row` (slotted: whole-window launches, see SplitSpec)
template <typename T>
__device__ __forceinline__ T* split_out(const SplitSpec& spec, int g, int64_t row, int col, int64_t n_rows) {
  const int64_t slot = spec.slot_rows > 0 ? div_small(row, spec.slot_rows, n_rows) : 0;
  return reinterpret_cast<T*>(static_cast<char*>(spec.dst[g]) + slot * spec.slot_stride) +
         (row - slot * spec.slot_rows) * spec.width[g] + col;
}

// One element, src -> dst. Equal dtypes are copied raw, as unsigned integers of their size (any 1/2/4/8-byte dtype,
// no rounding): Tout is then Tin, and integral; every other pair converts through float.
template <typename Tout, typename Tin>
__device__ __forceinline__ auto load_for(const Tin* s) {
  static_assert(!std::is_integral_v<Tout> || std::is_same_v<Tin, Tout>, "an integral output is a raw copy");
  if constexpr (std::is_integral_v<Tout>)
    return *s;
  else
    return Elem<Tin>::load1(s);
}
template <typename Tout, typename V>
__device__ __forceinline__ void store_as(Tout* d, V v) {
  static_assert(!std::is_integral_v<Tout> || std::is_same_v<V, Tout>, "an integral output is a raw copy");
  if constexpr (std::is_integral_v<Tout>)
    *d = v;
  else
    Elem<Tout>::store1(d, v);
}

template <typename Tin, typename Tout>
__global__ void __launch_bounds__(kThreads) split_columns_kernel(SplitSpec spec, const Tin* __restrict__ src,
                                                                 int64_t n_rows, int64_t n_values, RowIndex ri) {
  for_rows(n_rows, n_values, ri, [&](int64_t row, int col, int64_t src_row) {
    const auto v = load_for<Tout>(src + (src_row * n_values + col));
    const int g = group_of(spec, &col);
    store_as(split_out<Tout>(spec, g, row, col, n_rows), v);
  });
}

// ------------------------------------------------------------------- pack ---
// Inverse of split: k [n_src, w_g] groups -> one [n_rows, n_values] row block,
// row r taking source row source_row(ri, r) of every group (gather + concat +
// cast in one pass), in the same 64-row wave tiles: the output write is
// lane-contiguous, each group's reads are contiguous runs of w_g.
template <typename Tin, typename Tout>
__global__ void __launch_bounds__(kThreads) pack_columns_kernel(SplitSpec spec, Tout* __restrict__ dst,
                                                                int64_t n_rows, int64_t n_values, RowIndex ri) {
  for_rows(n_rows, n_values, ri, [&](int64_t row, int col, int64_t src_row) {
    Tout* d = dst + (row * n_values + col);
    const int g = group_of(spec, &col);
    store_as(d, load_for<Tout>(static_cast<const Tin*>(spec.dst[g]) + src_row * spec.width[g] + col));
  });
}

// What split_columns and pack_columns share: the argument checks, the grid of the row walk, and the (Tin, Tout) of
// the launch -- u8 / f32 / bf16 -> bf16 / f32, or for equal dtypes the unsigned integer of their size, twice.
template <typename F>
int launch_columns(const SplitSpec& spec, int32_t in_dt, int64_t n_rows, int64_t n_values, const RowIndex& ri,
                   F&& launch) {
  if (n_rows <= 0) return 0;
  if (!row_index_ok(ri, n_rows)) return -2;
  if (spec.n_groups < 1 || spec.n_groups > 8) return -2;
  if (n_values < 1 || n_values > (1 << 24)) return -2;  // 64 rows x n_values fits the tile's 32-bit walk
  int64_t blocks = (row_walk_waves(n_rows, n_values) + kThreads / 64 - 1) / (kThreads / 64);
  if (blocks > 8192) blocks = 8192;
  const dim3 grid(static_cast<uint32_t>(blocks));
  auto go = [&](auto in, auto out) {
    launch(grid, in, out);
    return static_cast<int>(hipGetLastError());
  };
  if (spec.out_dt == in_dt) {
    switch (dtype_size(in_dt)) {
      case 1: return go(uint8_t{}, uint8_t{});
      case 2: return go(uint16_t{}, uint16_t{});
      case 4: return go(uint32_t{}, uint32_t{});
      case 8: return go(uint64_t{}, uint64_t{});
    }
    return -1;
  }
  return with_dtype<kF32, kBF16, kU8>(in_dt, [&](auto in) {
    return with_dtype<kBF16, kF32>(spec.out_dt, [&](auto out) { return go(in, out); });
  });
}

}  // namespace

int collate_hwc_to_chw(void* dst, int32_t out_dt, const void* src, int32_t in_dt, int64_t batch, int64_t pixels,
                       int32_t channels, const RowIndex& ri, const Affine& aff, hipStream_t st) {
  if (batch <= 0 || pixels <= 0) return 0;
  if (!row_index_ok(ri, batch)) return -2;
  if (channels <= 0 || channels > kMaxAffineChannels) return -2;
  return with_dtype<kU8, kF32, kBF16>(in_dt, [&](auto in) {
    return with_dtype<kBF16, kF32>(out_dt, [&](auto out) {
      return launch_hwc<decltype(in), decltype(out)>(dst, src, batch, pixels, channels, ri, aff, st);
    });
  });
}

int split_columns(const SplitSpec& spec, const void* src, int32_t in_dt, int64_t n_rows, int64_t n_values,
                  const RowIndex& ri, hipStream_t st) {
  return launch_columns(spec, in_dt, n_rows, n_values, ri, [&](dim3 grid, auto in, auto out) {
    using Tin = decltype(in);
    hipLaunchKernelGGL((split_columns_kernel<Tin, decltype(out)>), grid, dim3(kThreads), 0, st, spec,
                       static_cast<const Tin*>(src), n_rows, n_values, ri);
  });
}

int pack_columns(const SplitSpec& spec, void* dst, int32_t in_dt, int64_t n_rows, int64_t n_values,
                 const RowIndex& ri, hipStream_t st) {
  return launch_columns(spec, in_dt, n_rows, n_values, ri, [&](dim3 grid, auto in, auto out) {
    using Tout = decltype(out);
    hipLaunchKernelGGL((pack_columns_kernel<decltype(in), Tout>), grid, dim3(kThreads), 0, st, spec,
                       static_cast<Tout*>(dst), n_rows, n_values, ri);
  });
}

}  // namespace ddl
