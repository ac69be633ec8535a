// Device only: the wave-level helpers of the token stream kernels (tokens_stream.hip, tokens_stream_rows.hip). The
// arithmetic they apply is tokens_stream.h; the host replays stand in for them with serial loops.
#pragma once

#include "common.h"
#include "tokens_stream.h"

namespace ddl {

// the `order` the per-lane routines of tokens_stream.h / tokens_stream_rows.h take: q = source_row(ri, position)
struct TsOrder {
  const RowIndex& ri;
  __device__ __forceinline__ int64_t operator()(int64_t i) const { return source_row(ri, i); }
};

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

}  // namespace ddl
