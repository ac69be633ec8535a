// Wave-level device helpers of the token stream kernels (tokens_stream.hip, tokens_stream_rows.hip) and the host
// check of a RowIndex both launchers make. HIP only; the arithmetic they apply is tokens_stream.h.
#pragma once

#include "common.h"
#include "tokens_stream.h"

namespace ddl {

__device__ __forceinline__ int64_t ts_wave_incl_scan(int64_t v) {
  const int lane = threadIdx.x & (kTpWave - 1);
#pragma unroll
  for (int d = 1; d < kTpWave; d <<= 1) {
    const int64_t u = __shfl_up(v, d, kTpWave);
    if (lane >= d) v += u;
  }
  return v;
}

__device__ __forceinline__ int64_t ts_wave_max(int64_t v) {
#pragma unroll
  for (int d = kTpWave / 2; d > 0; d >>= 1) {
    const int64_t u = __shfl_xor(v, d, kTpWave);
    v = u > v ? u : v;
  }
  return v;
}

// the last d in [0, n1) with table[d] <= v (table[0] <= v), by every wave on its own: no barrier
__device__ __forceinline__ int64_t ts_wave_last_le(const int64_t* table, int64_t n1, int64_t v) {
  const int lane = threadIdx.x & (kTpWave - 1);
  int64_t lo = 0, hi = n1;
  while (hi - lo > 1) {  // wave-uniform
    const int64_t stride = ts_search_stride(lo, hi);
    const int64_t p = ts_search_probe(lo, stride, lane);
    const bool le = p < hi && table[p] <= v;
    int k = __popcll(__ballot(le));
    if (k < 1) k = 1;  // lane 0 probes lo, which holds; kept so for a table that is not sorted
    ts_search_narrow(&lo, &hi, stride, k);
  }
  return lo;
}

// the checks of token_batch_descriptor on a RowIndex asked for positions [ri.base, ri.base + n)
inline bool ts_index_ok(const RowIndex& ri, int64_t n) {
  if (ri.mode < 0 || ri.mode > 2) return false;
  if (ri.mode == 1 && n > 0 && !ri.idx) return false;
  if (ri.mode != 1 && ri.base < 0) return false;
  if (ri.mode == 2) {  // every position inside the permutation's domain, and the domain inside the network's: the
                       // cycle walk of feistel_perm terminates only on a bijection
    const FeistelKeys& f = ri.keys;
    if (f.n == 0 || f.half_bits < 1 || f.half_bits > 32) return false;
    if (f.half_bits < 32 && f.n > (uint64_t{1} << (2 * f.half_bits))) return false;
    if (static_cast<uint64_t>(ri.base) + static_cast<uint64_t>(n) > f.n) return false;
  }
  return true;
}

}  // namespace ddl
