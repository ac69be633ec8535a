// Index arithmetic of the device ragged gather (ragged.hip), shared with host code: the host builds the
// tile map with it (ragged_tile_plan) and csrc/kernels/tests/ragged_index_check.cpp emulates the kernel
// tile by tile with it under ASan/UBSan. Plain inline functions: __host__ __device__ under hipcc, plain
// under g++ (this header includes nothing of HIP).
//
// A sequence of `len` elements of `eb` bytes starts at byte address `a` (only eb-aligned). Its source
// side is cut into UNITS: the naturally aligned 16-byte blocks of its aligned hull
//   [a & ~15, (a + len * eb + 15) & ~15).
// The first and the last unit may hold elements of the neighbouring sequences: they are loaded whole and
// masked. Element e of unit u is position p = u * (16 / eb) + e - head of the sequence, head = the
// elements of the first unit in front of `a`; it survives iff 0 <= p < len.
// A TILE is (sequence, chunk of kRgTileUnits units of its hull): one workgroup pass.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DDL_RG_HD __host__ __device__ __forceinline__
#else
#define DDL_RG_HD inline
#endif

namespace ddl {

constexpr int kRgThreads = 256;                      // lanes per workgroup
constexpr int kRgUnroll = 4;                         // independent 16 B loads per lane before its first store
constexpr int kRgUnitBytes = 16;                     // one lane's load
constexpr int kRgTileUnits = kRgThreads * kRgUnroll;  // 16 KB of source per tile

// first byte of the hull: the 16-byte block that holds byte address a
DDL_RG_HD uint64_t rg_hull_begin(uint64_t a) { return a & ~static_cast<uint64_t>(kRgUnitBytes - 1); }

// elements of the first unit that lie in front of the sequence (a is eb-aligned)
DDL_RG_HD int64_t rg_head_elems(uint64_t a, int eb) {
  return static_cast<int64_t>((a - rg_hull_begin(a)) / static_cast<uint64_t>(eb));
}

// units in the hull of `len` elements at byte address a (0 for an empty sequence: nothing is read)
DDL_RG_HD int64_t rg_units(uint64_t a, int64_t len, int eb) {
  if (len <= 0) return 0;
  const uint64_t end = a + static_cast<uint64_t>(len) * static_cast<uint64_t>(eb);
  const uint64_t hull_end = (end + (kRgUnitBytes - 1)) & ~static_cast<uint64_t>(kRgUnitBytes - 1);
  return static_cast<int64_t>((hull_end - rg_hull_begin(a)) / kRgUnitBytes);
}

DDL_RG_HD int64_t rg_tiles(int64_t units) { return (units + kRgTileUnits - 1) / kRgTileUnits; }

// unit that lane `tid` loads in round k of chunk `chunk` (consecutive lanes: consecutive units)
DDL_RG_HD int64_t rg_unit(int64_t chunk, int k, int tid) {
  return chunk * kRgTileUnits + static_cast<int64_t>(k) * kRgThreads + tid;
}

// byte address of unit u of the hull of a sequence at a (16-byte aligned by construction)
DDL_RG_HD uint64_t rg_unit_addr(uint64_t a, int64_t u) {
  return rg_hull_begin(a) + static_cast<uint64_t>(u) * kRgUnitBytes;
}

// position in the sequence of element e of unit u (negative: in front of the sequence)
DDL_RG_HD int64_t rg_elem_pos(int64_t u, int e, int64_t head, int eb) {
  return u * (kRgUnitBytes / eb) + e - head;
}

// sequence of tile `tile`: the last i with tile_start[i] <= tile. tile_start[0] = 0, tile < tile_start[n],
// so 0 <= i < n and tile < tile_start[i + 1]: sequence i has tiles (it is not empty) and holds this one.
template <typename At>
DDL_RG_HD int64_t rg_find_seq(At at, int64_t n, int64_t tile) {
  int64_t lo = 0, hi = n + 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(at(mid)) <= tile)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - 1;
}

// Host: tile_start[0..n] for n sequences (src_start[i] elements into the source at byte address src,
// lengths dst_offsets[i + 1] - dst_offsets[i]); returns the tile count, or -1 if it does not fit int32.
inline int64_t ragged_tile_plan(uint64_t src, const int64_t* src_start, const int64_t* dst_offsets, int64_t n, int eb,
                                int32_t* tile_start) {
  int64_t t = 0;
  tile_start[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t a = src + static_cast<uint64_t>(src_start[i]) * static_cast<uint64_t>(eb);
    t += rg_tiles(rg_units(a, dst_offsets[i + 1] - dst_offsets[i], eb));
    if (t > INT32_MAX) return -1;
    tile_start[i + 1] = static_cast<int32_t>(t);
  }
  return t;
}

}  // namespace ddl
