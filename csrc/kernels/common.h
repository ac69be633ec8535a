// Shared device/host helpers for the ddl_amd CDNA4 (gfx950) kernels.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)  // host check programs (csrc/kernels/tests) include this header without HIP
#include <hip/hip_runtime.h>
#define DDL_HD __host__ __device__ __forceinline__
#else
#define DDL_HD inline
#endif

namespace ddl {

// ---------------------------------------------------------------------------
// Counter-based pseudo-random permutation of [0, n): a 6-round balanced
// Feistel network over 2^(2h) >= n with cycle walking. perm(i) is a pure
// function of (keys, n, i): no sort, no materialised table, bit-identical on
// host (ddl_amd/permutation.py mirrors it in numpy) and device, and
// independent of how many ranks ask for which positions -- the basis of the
// world-size-invariant epoch order. Replaces the reference's
// per-producer rank-seeded rng.shuffle (reference tests/run_ddl.py:122,167).
constexpr int kFeistelRounds = 6;

struct FeistelKeys {
  uint64_t k[kFeistelRounds];
  uint64_t n;          // domain size (rows)
  uint32_t half_bits;  // h: the network permutes [0, 2^(2h))
  uint32_t pad;
};

DDL_HD uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

DDL_HD uint64_t feistel_once(uint64_t x, const FeistelKeys& f) {
  const uint64_t mask = (1ull << f.half_bits) - 1ull;
  uint64_t l = x >> f.half_bits, r = x & mask;
#pragma unroll
  for (int i = 0; i < kFeistelRounds; ++i) {
    const uint64_t t = l ^ (mix64(r ^ f.k[i]) & mask);
    l = r;
    r = t;
  }
  return (l << f.half_bits) | r;
}

DDL_HD uint64_t feistel_perm(uint64_t i, const FeistelKeys& f) {
  uint64_t x = feistel_once(i, f);
  while (x >= f.n) x = feistel_once(x, f);  // cycle walk: terminates (bijection)
  return x;
}

// How a gather kernel finds the source row of output row r.
struct RowIndex {
  const int64_t* idx;  // explicit indices (device or host-mapped), or null
  int64_t base;        // src row = perm(base + r) (or idx[r] + 0 when idx != null)
  int32_t mode;        // 0: identity (base + r), 1: explicit idx, 2: feistel perm
  int32_t pad;
  FeistelKeys keys;
};

DDL_HD int64_t source_row(const RowIndex& ri, int64_t r) {
  if (ri.mode == 1) return ri.idx[r];
  if (ri.mode == 2) return static_cast<int64_t>(feistel_perm(static_cast<uint64_t>(ri.base + r), ri.keys));
  return ri.base + r;
}

// Host check every launcher whose kernels evaluate source_row(ri, 0 .. n) makes before it launches anything (the row
// launchers of permute / collate / augment.hip and the token planners alike; a failure is the argument error -2):
// a known mode, an index vector in mode 1, no negative position, and in mode 2 every position inside the
// permutation's domain and the domain inside the network's -- the cycle walk of feistel_perm terminates only on a
// bijection.
inline bool row_index_ok(const RowIndex& ri, int64_t n) {
  if (ri.mode < 0 || ri.mode > 2) return false;
  if (ri.mode == 1 && n > 0 && !ri.idx) return false;
  if (ri.mode != 1 && ri.base < 0) return false;
  if (ri.mode == 2) {
    const FeistelKeys& f = ri.keys;
    if (f.n == 0 || f.half_bits < 1 || f.half_bits > 32) return false;
    if (f.half_bits < 32 && f.n > (uint64_t{1} << (2 * f.half_bits))) return false;
    if (static_cast<uint64_t>(ri.base) + static_cast<uint64_t>(n) > f.n) return false;
  }
  return true;
}

// Per-channel affine epilogue (normalisation) fused into gathers / casts:
// out = in * scale[ch] + bias[ch], ch = (element_in_row / plane) % channels.
constexpr int kMaxAffineChannels = 16;
struct Affine {
  float scale[kMaxAffineChannels];
  float bias[kMaxAffineChannels];
  int64_t plane;    // elements per channel plane (H*W for images, 1 for per-column tables)
  int32_t channels; // <= kMaxAffineChannels
  int32_t enabled;
};

// dtype codes shared with the Python side (ddl_amd/ops/_dtypes.py)
enum DType : int32_t { kU8 = 0, kI32 = 1, kI64 = 2, kF16 = 3, kBF16 = 4, kF32 = 5 };

inline int dtype_size(int32_t d) {
  switch (d) {
    case kU8: return 1;
    case kF16: case kBF16: return 2;
    case kI32: case kF32: return 4;
    case kI64: return 8;
  }
  return 0;
}

}  // namespace ddl
