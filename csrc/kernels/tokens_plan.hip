// Batch descriptor of the HBM-resident token loader, built on the device: "positions [base, base + n) of the
// epoch order" -> src_start / offsets / seg_src, the inputs of pack_plan_device (tokens.hip) and
// pad_pack_tokens_indexed (tokens_indexed.hip). With it a step's host work is launches: no index vector, no
// cumulative sum, no H2D copy.
//
// Shape: pack_plan_kernel's, which it feeds. One workgroup of 1024 lanes walks the batch in 1024-wide tiles;
// lane t of a tile evaluates its sequence's index (the Feistel permutation inline, an explicit device index, or
// base + i), loads the sequence's two corpus offsets and takes part in two wave scans (__shfl_up) -- the tokens
// and the segments in front of it -- joined through one total per wave in LDS and carried from tile to tile.
// The longest segment is a wave maximum (__shfl_xor) folded by lane 0. Every exit and barrier is
// block-uniform; nothing is an atomic. At 2048 sequences the kernel is two tiles: a latency chain of one
// workgroup, not a bandwidth problem. All the index arithmetic is tokens_plan.h.
//
// Bounded reads: corpus_offsets[q] and corpus_offsets[q + 1] are read only for 0 <= q < n_corpus; an index
// outside that range -- a corrupt index vector -- is not dereferenced, the sequence counts as empty (src_start
// 0, no token, no segment). An explicit index is read at [0, n). Nothing of the corpus itself is read.
// Bounded writes: src_start[0 .. n), offsets[0 .. n], counts[2 .. 3] (and counts[0 .. 1] with pad_counts, when
// no plan kernel follows), each exactly once; seg_src[k] only for k < max_segs: a batch with more segments
// than the capacity writes nothing past it and is left for pack_plan_kernel to report (counts[0] = -1).
#include "common.h"
#include "launch.h"
#include "tokens_plan.h"

namespace ddl {
namespace {

__device__ __forceinline__ int64_t tp_wave_incl_scan(int64_t v) {
  const int lane = threadIdx.x & (kTpWave - 1);
#pragma unroll
  for (int d = 1; d < kTpWave; d <<= 1) {
    const int64_t u = __shfl_up(v, d, kTpWave);
    if (lane >= d) v += u;
  }
  return v;
}

__device__ __forceinline__ int64_t tp_wave_max(int64_t v) {
#pragma unroll
  for (int d = kTpWave / 2; d > 0; d >>= 1) {
    const int64_t u = __shfl_xor(v, d, kTpWave);
    v = u > v ? u : v;
  }
  return v;
}

__global__ void __launch_bounds__(kTpThreads) token_batch_descriptor_kernel(BatchDescSpec sp) {
  __shared__ int64_t wave_tok[kTpWaves], wave_seg[kTpWaves], wave_max[kTpWaves];
  __shared__ int64_t carry_tok, carry_seg, carry_max;
  const int t = threadIdx.x, lane = t & (kTpWave - 1), wv = t / kTpWave;
  const int64_t S = sp.seq_len;
  if (t == 0) carry_tok = carry_seg = carry_max = 0;
  __syncthreads();
  for (int64_t b = 0; b < sp.n; b += kTpThreads) {  // block-uniform trip count
    const int64_t i = b + t;
    int64_t s0 = 0, len = 0;
    if (i < sp.n) {
      const int64_t q = source_row(sp.ri, i);
      if (tp_index_ok(q, sp.n_corpus)) {
        s0 = sp.corpus_offsets[q];
        len = tp_len(s0, sp.corpus_offsets[q + 1]);
      }
    }
    const int64_t c = tp_seg_count(len, S);
    const int64_t incl_tok = tp_wave_incl_scan(len);
    const int64_t incl_seg = tp_wave_incl_scan(c);
    const int64_t mx = tp_wave_max(tp_seg_max(len, S));
    if (lane == kTpWave - 1) {
      wave_tok[wv] = incl_tok;
      wave_seg[wv] = incl_seg;
      wave_max[wv] = mx;
    }
    __syncthreads();
    const int64_t before_tok = tp_before(wave_tok, wv, carry_tok);
    const int64_t before_seg = tp_before(wave_seg, wv, carry_seg);
    if (i < sp.n) {
      sp.src_start[i] = s0;
      sp.offsets[i] = tp_exclusive(before_tok, incl_tok, len);
    }
    const int64_t first = tp_exclusive(before_seg, incl_seg, c);
    const int64_t cnt = tp_seg_writes(first, c, sp.max_segs);
    for (int64_t j = 0; j < cnt; ++j) sp.seg_src[first + j] = tp_seg_src(s0, j, S);
    __syncthreads();  // every lane has read the carries and the wave totals
    if (t == kTpThreads - 1) {
      carry_tok = before_tok + incl_tok;
      carry_seg = before_seg + incl_seg;
    }
    if (t == 0) {
      int64_t m = carry_max;
      for (int k = 0; k < kTpWaves; ++k) m = wave_max[k] > m ? wave_max[k] : m;
      carry_max = m;
    }
    __syncthreads();
  }
  if (t == 0) {
    sp.offsets[sp.n] = carry_tok;
    sp.counts[2] = carry_tok;
    sp.counts[3] = carry_max;
    if (sp.pad_counts) {  // pad mode: no plan kernel owns slots 0 and 1
      sp.counts[0] = sp.n;
      sp.counts[1] = 0;
    }
  }
}

}  // namespace

int token_batch_descriptor(const BatchDescSpec& spec, hipStream_t st) {
  if (spec.n < 0 || spec.seq_len <= 0 || spec.max_segs < 0 || spec.n_corpus < 0) return -2;
  if (!spec.src_start || !spec.offsets || !spec.counts) return -2;
  if (spec.max_segs > 0 && !spec.seg_src) return -2;
  if (spec.n_corpus > 0 && !spec.corpus_offsets) return -2;
  if (!row_index_ok(spec.ri, spec.n)) return -2;
  hipLaunchKernelGGL(token_batch_descriptor_kernel, dim3(1), dim3(kTpThreads), 0, st, spec);
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
