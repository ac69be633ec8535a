// Row gather / permute / scatter kernels with fused dtype cast and per-channel
// normalisation.
//
// One kernel family serves every "move rows by index" need of the loader:
//   * the global-shuffle permutation of a window resident in HBM (the
//     reference's rng.shuffle of the producer window, tests/run_ddl.py:167,
//     now an out-of-place device gather -- each row read once, written once),
//   * gather/scatter of the rows exchanged between GPUs over RCCL
//     (reference ddl/shuffle.py:92-108),
//   * zero-copy gathers straight out of pinned, device-mapped host memory.
// The source row of output row r comes from RowIndex: identity, an explicit
// index vector, or the counter-based Feistel permutation computed inline.
//
// Memory-bound: every lane moves 16 B per access (guide G13), 4 independent
// accesses in flight per lane, one row chunk per workgroup so a 301 KB image
// row becomes ~19 workgroups (thousands of workgroups per batch >> 256 CUs).
#include "elem.h"
#include "launch.h"

namespace ddl {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kUnroll = 4;

// ------------------------------ raw byte moves ------------------------------
// Load policy: non-temporal loads of the gathered source rows (below). Store policy of the raw row moves:
// plain stores, which leave the batch in the 256 MB MALL for a consumer
// that reads it right away. Streaming stores measured +7.8% on the isolated 1024-image gather (5.39 vs 5.00
// TB/s) but 5.49M vs 5.74M samples/s in the HBM-resident loader, which reads the batch right after it is
// written (profiles/r4_second/resident_*.json): plain stores only.

template <typename U, bool kNtLoads>
__global__ void __launch_bounds__(kThreads) move_rows_chunked(uint8_t* __restrict__ dst,
                                                              const uint8_t* __restrict__ src,
                                                              int64_t units_per_row, int64_t chunks_per_row,
                                                              int64_t n_tiles, RowIndex ri, int scatter) {
  // Grid-stride over (row, chunk) tiles: normally one tile per workgroup; a capped
  // grid (zero-copy host gathers) keeps the PCIe-latency-bound kernel on few CUs.
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const auto [row, chunk] = row_chunk(tile, chunks_per_row);
    const int64_t mapped = source_row(ri, row);
    const int64_t srow = scatter ? row : mapped;
    const int64_t drow = scatter ? mapped : row;
    const U* s = reinterpret_cast<const U*>(src) + srow * units_per_row;
    U* d = reinterpret_cast<U*>(dst) + drow * units_per_row;
    const int64_t u0 = chunk * (kThreads * kUnroll) + threadIdx.x;
    U v[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int64_t u = u0 + k * kThreads;
      // kNtLoads (gathers): the source rows stream through once (a shard far larger than the 256 MB MALL):
      // non-temporal loads keep them from evicting the batch just written, which the consumer reads next (the
      // HBM-resident loader: bf16 5.50 -> 6.04M samples/s, kernel 5.00 -> 5.20 TB/s; profiles/r5_configs/
      // nt_loads/). Scatters read a contiguous receive buffer: plain loads (non-temporal there: 5.01 -> 4.91).
      // A template flag, not a runtime select: the compiler merges `c ? s[u] : nt_load(s + u)` into one plain load.
      if (u < units_per_row) {
        if constexpr (kNtLoads)
          v[k] = __builtin_nontemporal_load(s + u);
        else
          v[k] = s[u];
      }
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int64_t u = u0 + k * kThreads;
      if (u < units_per_row) {
        d[u] = v[k];
      }
    }
  }
}

template <typename U>
__global__ void __launch_bounds__(kThreads) move_rows_flat(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src,
                                                           int64_t units_per_row, int64_t total_units, RowIndex ri,
                                                           int scatter) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; u < total_units; u += stride) {
    const int64_t row = div_small(u, units_per_row, total_units);
    const int64_t col = u - row * units_per_row;
    const int64_t mapped = source_row(ri, row);
    const int64_t srow = scatter ? row : mapped;
    const int64_t drow = scatter ? mapped : row;
    reinterpret_cast<U*>(dst)[drow * units_per_row + col] =
        reinterpret_cast<const U*>(src)[srow * units_per_row + col];
  }
}

// ------------------------------ converting moves ----------------------------
// Channel of in-row element `elem`. Rows hold < 2^31 elements (checked on the host), so this is
// 32-bit unsigned division (a short v_rcp_iflag sequence) instead of the long 64-bit expansion.
__device__ __forceinline__ int affine_channel(const Affine& a, int64_t elem) {
  return static_cast<int>((static_cast<uint32_t>(elem) / static_cast<uint32_t>(a.plane)) %
                          static_cast<uint32_t>(a.channels));
}

__device__ __forceinline__ void apply_affine(const Affine& a, int64_t elem, float (&f)[8]) {
  if (!a.enabled) return;
  // 8 consecutive elements share a channel when plane % 8 == 0 (checked on host).
  const int ch = affine_channel(a, elem);
  // <= 4 channels (RGB / RGBA): select among values loaded with constant indices
  // (scalar kernel-argument loads) instead of a per-lane dynamic load.
  float s, b;
  if (a.channels <= 4) {
    const float s0 = a.scale[0], s1 = a.scale[1], s2 = a.scale[2], s3 = a.scale[3];
    const float b0 = a.bias[0], b1 = a.bias[1], b2 = a.bias[2], b3 = a.bias[3];
    s = ch == 0 ? s0 : (ch == 1 ? s1 : (ch == 2 ? s2 : s3));
    b = ch == 0 ? b0 : (ch == 1 ? b1 : (ch == 2 ? b2 : b3));
  } else {
    s = a.scale[ch];
    b = a.bias[ch];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = fmaf(f[i], s, b);
}

template <typename Tin, typename Tout>
__global__ void __launch_bounds__(kThreads) convert_rows_chunked(Tout* __restrict__ dst, const Tin* __restrict__ src,
                                                                 int64_t row_elems, int64_t chunks_per_row,
                                                                 int64_t n_tiles, RowIndex ri, Affine aff) {
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const auto [row, chunk] = row_chunk(tile, chunks_per_row);
    const int64_t srow = source_row(ri, row);
    const Tin* s = src + srow * row_elems;
    Tout* d = dst + row * row_elems;
    const int64_t e0 = (chunk * (kThreads * kUnroll) + threadIdx.x) * 8;
    float f[kUnroll][8];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int64_t e = e0 + static_cast<int64_t>(k) * kThreads * 8;
      if (e < row_elems) Elem<Tin>::load8(s + e, f[k]);
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int64_t e = e0 + static_cast<int64_t>(k) * kThreads * 8;
      if (e < row_elems) {
        apply_affine(aff, e, f[k]);
        Elem<Tout>::template store<8>(d + e, f[k]);
      }
    }
  }
}

// uint8 sources: 8 elements (8 B) per lane per load, 8 outputs (16 B of bf16) per
// lane per store, so every load AND every store instruction of a wave covers one
// contiguous span (512 B in, 1 KB out). (16 B u8 loads -> 2 x 16 B stores left
// each store instruction with 16 B holes between lanes: 85-87% of HBM.) The
// kU raw loads are all issued before any conversion: the kernel is bound by
// bytes in flight per CU (16 KB of loads per workgroup).
constexpr int kU8Loads = 8;

template <typename Tout, bool kNtLoads>
__global__ void __launch_bounds__(kThreads) convert_u8_rows_chunked(Tout* __restrict__ dst,
                                                                    const uint8_t* __restrict__ src, int64_t row_elems,
                                                                    int64_t chunks_per_row, int64_t n_tiles, RowIndex ri,
                                                                    Affine aff) {
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const auto [row, chunk] = row_chunk(tile, chunks_per_row);
    const int64_t srow = source_row(ri, row);
    const uint8_t* s = src + srow * row_elems;
    Tout* d = dst + row * row_elems;
    const int64_t e0 = (chunk * (kThreads * kU8Loads) + threadIdx.x) * 8;
    uint2 raw[kU8Loads];
#pragma unroll
    for (int k = 0; k < kU8Loads; ++k) {
      const int64_t e = e0 + static_cast<int64_t>(k) * kThreads * 8;
      if (e < row_elems) {  // non-temporal for device sources, as in move_rows_chunked (uint8 resident loader
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));  // 5.99 -> 6.21M samples/s)
        const u32x2 t = kNtLoads ? __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(s + e))
                                 : *reinterpret_cast<const u32x2*>(s + e);
        raw[k] = make_uint2(t.x, t.y);
      } else {
        raw[k] = uint2{};
      }
    }
#pragma unroll
    for (int k = 0; k < kU8Loads; ++k) {
      const int64_t e = e0 + static_cast<int64_t>(k) * kThreads * 8;
      if (e < row_elems) {
        float f[8];
        unpack_u8x8(raw[k].x, raw[k].y, f);
        apply_affine(aff, e, f);
        Elem<Tout>::template store<8>(d + e, f);
      }
    }
  }
}

template <typename Tin, typename Tout>
__global__ void __launch_bounds__(kThreads) convert_rows_flat(Tout* __restrict__ dst, const Tin* __restrict__ src,
                                                              int64_t row_elems, int64_t total, RowIndex ri, Affine aff) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; e < total; e += stride) {
    const int64_t row = div_small(e, row_elems, total);
    const int64_t col = e - row * row_elems;
    float v = Elem<Tin>::load1(src + source_row(ri, row) * row_elems + col);
    if (aff.enabled) {
      const int ch = affine_channel(aff, col);
      v = fmaf(v, aff.scale[ch], aff.bias[ch]);
    }
    Elem<Tout>::store1(dst + e, v);
  }
}

int flat_grid(int64_t work) {
  const int64_t blocks = (work + kThreads - 1) / kThreads;
  return static_cast<int>(blocks < 4096 ? (blocks < 1 ? 1 : blocks) : 4096);
}

dim3 tile_grid(int64_t n_tiles, int64_t max_blocks) {
  const int64_t g = (max_blocks > 0 && max_blocks < n_tiles) ? max_blocks : n_tiles;
  return dim3(static_cast<uint32_t>(g));
}

int flat_grid_capped(int64_t work, int64_t max_blocks) {
  const int g = flat_grid(work);
  return (max_blocks > 0 && max_blocks < g) ? static_cast<int>(max_blocks) : g;
}

template <typename U>
int launch_move(void* dst, const void* src, int64_t n_rows, int64_t row_bytes, const RowIndex& ri, int scatter,
                bool nt_loads, int64_t max_blocks, hipStream_t st) {
  const int64_t units = row_bytes / static_cast<int64_t>(sizeof(U));
  if (units >= kThreads) {
    const int64_t chunks = (units + kThreads * kUnroll - 1) / (kThreads * kUnroll);
    // move_rows_chunked divides the tile number in 32 bits. gather_rows' bound on n_rows * row_elems does not
    // imply this one: chunks <= units / 256 only gives n_tiles < 2^40 * (element size / unit size) / 256, and
    // e.g. 2^30 rows of 513 int64 (1026 4-byte units, 2 chunks) pass that bound with 2^31 tiles.
    if (n_rows * chunks >= (int64_t{1} << 31)) return -4;
    auto kernel = nt_loads ? move_rows_chunked<U, true> : move_rows_chunked<U, false>;
    hipLaunchKernelGGL(kernel, tile_grid(n_rows * chunks, max_blocks), dim3(kThreads), 0, st,
                       static_cast<uint8_t*>(dst), static_cast<const uint8_t*>(src), units, chunks, n_rows * chunks,
                       ri, scatter);
  } else {
    hipLaunchKernelGGL(move_rows_flat<U>, dim3(flat_grid_capped(n_rows * units, max_blocks)), dim3(kThreads), 0, st,
                       static_cast<uint8_t*>(dst), static_cast<const uint8_t*>(src), units, n_rows * units, ri,
                       scatter);
  }
  return static_cast<int>(hipGetLastError());
}

template <typename Tin, typename Tout>
void launch_convert(void* dst, const void* src, int64_t n_rows, int64_t row_elems, const RowIndex& ri, const Affine& aff,
                    bool vec_ok, bool nt_loads, int64_t max_blocks, hipStream_t st) {
  if constexpr (std::is_same_v<Tin, uint8_t>) {
    if (vec_ok && row_elems >= kThreads * 8) {  // vec_ok: row_elems % 8 == 0, 16 B aligned
      const int64_t chunks = (row_elems + kThreads * kU8Loads * 8 - 1) / (kThreads * kU8Loads * 8);
      auto kernel = nt_loads ? convert_u8_rows_chunked<Tout, true> : convert_u8_rows_chunked<Tout, false>;
      hipLaunchKernelGGL(kernel, tile_grid(n_rows * chunks, max_blocks), dim3(kThreads), 0,
                         st, static_cast<Tout*>(dst), static_cast<const uint8_t*>(src), row_elems, chunks,
                         n_rows * chunks, ri, aff);
      return;
    }
  }
  if (vec_ok && row_elems >= kThreads * 8) {
    const int64_t chunks = (row_elems + kThreads * kUnroll * 8 - 1) / (kThreads * kUnroll * 8);
    hipLaunchKernelGGL((convert_rows_chunked<Tin, Tout>), tile_grid(n_rows * chunks, max_blocks), dim3(kThreads), 0,
                       st, static_cast<Tout*>(dst), static_cast<const Tin*>(src), row_elems, chunks, n_rows * chunks,
                       ri, aff);
  } else {
    hipLaunchKernelGGL((convert_rows_flat<Tin, Tout>), dim3(flat_grid_capped(n_rows * row_elems, max_blocks)),
                       dim3(kThreads), 0, st,
                       static_cast<Tout*>(dst), static_cast<const Tin*>(src), row_elems, n_rows * row_elems, ri, aff);
  }
}

__global__ void __launch_bounds__(kThreads) feistel_fill(int64_t* __restrict__ out, int64_t count, int64_t base,
                                                         FeistelKeys keys) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < count; i += stride)
    out[i] = static_cast<int64_t>(feistel_perm(static_cast<uint64_t>(base + i), keys));
}

}  // namespace

int gather_rows(void* dst, int32_t out_dt, const void* src, int32_t in_dt, int64_t n_rows, int64_t row_elems,
                const RowIndex& ri, const Affine& aff, int flags, int64_t max_blocks, hipStream_t st) {
  if (n_rows <= 0 || row_elems <= 0) return 0;
  if (!row_index_ok(ri, n_rows)) return -2;
  const int scatter = flags & 1;
  const bool nt = (flags & (1 | kHostSource)) == 0;  // a device-source gather: non-temporal source loads
  // the chunked kernels index tiles and in-row elements with 32-bit arithmetic. The converting ones take rows of
  // >= 2048 elements in chunks of >= 8192, so chunks <= row_elems / 2048 and their tiles stay below 2^29 under
  // this bound; the raw moves' tile count depends on the unit width and is checked in launch_move.
  if (n_rows >= (int64_t{1} << 31) || n_rows * row_elems >= (int64_t{1} << 40)) return -4;
  const bool same = (out_dt == in_dt) && !aff.enabled;
  if (same) {
    const int64_t row_bytes = row_elems * dtype_size(in_dt);
    const uintptr_t align = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);
    if (row_bytes % 16 == 0 && align % 16 == 0)
      return launch_move<u32x4>(dst, src, n_rows, row_bytes, ri, scatter, nt, max_blocks, st);
    if (row_bytes % 4 == 0 && align % 4 == 0)
      return launch_move<uint32_t>(dst, src, n_rows, row_bytes, ri, scatter, nt, max_blocks, st);
    return launch_move<uint8_t>(dst, src, n_rows, row_bytes, ri, scatter, nt, max_blocks, st);
  }
  if (scatter) return -2;  // converting scatters are not needed by the loader
  if (row_elems >= (int64_t{1} << 31) || (aff.enabled && aff.plane >= (int64_t{1} << 31))) return -4;
  const uintptr_t align = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);
  bool vec_ok = (row_elems % 8 == 0) && (align % 16 == 0);
  if (aff.enabled && (aff.plane % 8 != 0)) vec_ok = false;
  const int rc = with_dtype<kU8, kF32, kBF16, kF16>(in_dt, [&](auto in) {
    return with_dtype<kBF16, kF16, kF32>(out_dt, [&](auto out) {
      launch_convert<decltype(in), decltype(out)>(dst, src, n_rows, row_elems, ri, aff, vec_ok, nt, max_blocks, st);
      return 0;
    });
  });
  if (rc != 0) return -3;
  return static_cast<int>(hipGetLastError());
}

int feistel_indices(int64_t* out, int64_t count, int64_t base, const FeistelKeys& keys, hipStream_t st) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(feistel_fill, dim3(flat_grid(count)), dim3(kThreads), 0, st, out, count, base, keys);
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
