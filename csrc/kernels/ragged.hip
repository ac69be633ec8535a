// Device ragged gather: the twin of the host gather_ragged (csrc/runtime/arena.cpp). Sequence i of a flat
// token array (2- or 4-byte elements), src_start[i] elements in, is copied to dst[dst_offsets[i] ..
// dst_offsets[i + 1]). The source may be pinned, device-mapped host memory (the zero-copy token loader:
// every byte crosses PCIe exactly once) or HBM; the destination is HBM.
//
// The source side decides the shape. Mapped host memory is uncached on the device, so every load
// instruction is a PCIe read: each lane issues naturally aligned 16-byte non-temporal loads, kRgUnroll of
// them before its first store (16 KB per workgroup in flight; the link needs ~110 KB). Sequence starts
// are only element-aligned, so the alignment is taken on the source: a sequence is read as the 16-byte
// units of its aligned hull (ragged_index.h), the first and last unit loaded whole and masked. The
// destination is HBM at ~100 x the link rate: the surviving elements go out as per-element stores.
//
// Bounded reads: the kernel reads nothing outside the 16-byte aligned hull of the sequences it copies. A
// naturally aligned 16-byte load never crosses a page, and the loader registers the page-rounded mapping
// of the corpus, so every byte of a hull lies in a page that holds a byte of its sequence: it is mapped.
// An empty sequence has no units and no tile: nothing of it is read.
// Bounded writes: element p of sequence i is stored only for 0 <= p < len_i, at dst[dst_offsets[i] + p]
// < dst[dst_offsets[n]].
//
// Tiles are (sequence, chunk of kRgTileUnits units); workgroups grid-stride over them (max_blocks caps
// the grid: the kernel is link-latency-bound and should leave the CUs to the training step). The tile ->
// sequence map is the host-built prefix tile_start[n + 1], staged in LDS when n <= kRgMapCap and searched
// in global memory otherwise. All byte offsets are 64-bit (a corpus is larger than 4 GB).
#include "common.h"
#include "launch.h"
#include "ragged_index.h"

namespace ddl {
namespace {

constexpr int kRgMapCap = kRaggedMapCap;  // sequences whose tile map is staged in LDS (8 KB of int32)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ T unit_elem(const u32x4& v, int e) {
  constexpr int per_word = 4 / static_cast<int>(sizeof(T));
  const uint32_t w = v[e / per_word];
  if constexpr (sizeof(T) == 4)
    return w;
  else
    return static_cast<T>(w >> (16 * (e % per_word)));
}

template <typename T>
__global__ void __launch_bounds__(kRgThreads) gather_ragged_kernel(T* __restrict__ dst, const uint8_t* __restrict__ src,
                                                                   const int64_t* __restrict__ src_start,
                                                                   const int64_t* __restrict__ dst_offsets,
                                                                   const int32_t* __restrict__ tile_start, int64_t n,
                                                                   int64_t n_tiles) {
  constexpr int eb = static_cast<int>(sizeof(T));
  constexpr int per_unit = kRgUnitBytes / eb;
  __shared__ int32_t map_lds[kRgMapCap + 1];
  const bool in_lds = n <= kRgMapCap;  // kernel argument: block-uniform
  if (in_lds) {
    for (int64_t i = threadIdx.x; i <= n; i += kRgThreads) map_lds[i] = tile_start[i];
    __syncthreads();
  }
  const int tid = static_cast<int>(threadIdx.x);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t seq = in_lds ? rg_find_seq([&](int64_t j) { return map_lds[j]; }, n, tile)
                               : rg_find_seq([&](int64_t j) { return tile_start[j]; }, n, tile);
    const int64_t chunk = tile - (in_lds ? map_lds[seq] : tile_start[seq]);
    const int64_t d0 = dst_offsets[seq];
    const int64_t len = dst_offsets[seq + 1] - d0;
    const uint64_t a = reinterpret_cast<uint64_t>(src) + static_cast<uint64_t>(src_start[seq]) * eb;
    const int64_t units = rg_units(a, len, eb);
    const int64_t head = rg_head_elems(a, eb);
    u32x4 v[kRgUnroll];
#pragma unroll
    for (int k = 0; k < kRgUnroll; ++k) {
      const int64_t u = rg_unit(chunk, k, tid);
      // the unit's address as an offset from the kernel argument (negative in a first unit in front of an
      // unaligned src), so the load stays a global one
      if (u < units)
        v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(
            src + static_cast<int64_t>(rg_unit_addr(a, u) - reinterpret_cast<uint64_t>(src))));
    }
#pragma unroll
    for (int k = 0; k < kRgUnroll; ++k) {
      const int64_t u = rg_unit(chunk, k, tid);
      if (u < units) {
        T* d = dst + d0;
#pragma unroll
        for (int e = 0; e < per_unit; ++e) {
          const int64_t p = rg_elem_pos(u, e, head, eb);
          if (p >= 0 && p < len) d[p] = unit_elem<T>(v[k], e);
        }
      }
    }
  }
}

}  // namespace

int gather_ragged(void* dst, const void* src, const int64_t* src_start, const int64_t* dst_offsets,
                  const int32_t* tile_start, int64_t n, int64_t n_tiles, int elem_bytes, int64_t max_blocks,
                  hipStream_t st) {
  if (elem_bytes != 2 && elem_bytes != 4) return -1;
  if (n < 0 || n_tiles < 0 || n_tiles > INT32_MAX) return -4;
  if (n == 0 || n_tiles == 0) return 0;  // nothing to copy: no launch
  if (reinterpret_cast<uintptr_t>(src) % elem_bytes || reinterpret_cast<uintptr_t>(dst) % elem_bytes) return -2;
  const int64_t g = (max_blocks > 0 && max_blocks < n_tiles) ? max_blocks : n_tiles;
  const dim3 grid(static_cast<uint32_t>(g));
  if (elem_bytes == 4)
    hipLaunchKernelGGL(gather_ragged_kernel<uint32_t>, grid, dim3(kRgThreads), 0, st, static_cast<uint32_t*>(dst),
                       static_cast<const uint8_t*>(src), src_start, dst_offsets, tile_start, n, n_tiles);
  else
    hipLaunchKernelGGL(gather_ragged_kernel<uint16_t>, grid, dim3(kRgThreads), 0, st, static_cast<uint16_t*>(dst),
                       static_cast<const uint8_t*>(src), src_start, dst_offsets, tile_start, n, n_tiles);
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
