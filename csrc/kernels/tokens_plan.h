// Index arithmetic of the batch descriptor kernel (tokens_plan.hip), shared with host code:
// csrc/kernels/tests/tokens_plan_check.cpp replays the kernel's per-lane loops with it under ASan/UBSan (the
// harness of all the checks is tests/check_common.h).
// Plain inline functions: __host__ __device__ under hipcc, plain under g++ (this header includes nothing of HIP).
//
// The kernel turns the n selected sequences of a corpus (sequence q = corpus elements
// [corpus_offsets[q], corpus_offsets[q + 1])) into the inputs of pack_plan_device and pad_pack_tokens_indexed:
//   src_start[i]  = corpus_offsets[q_i]
//   offsets[i]    = sum of len_k, k < i            (the virtual flat stream; offsets[n] = the token count)
//   seg_src[f_i + j] = src_start[i] + j * S,  j < c_i = ceil(len_i / S),  f_i = sum of c_k, k < i
// One workgroup of kTpThreads lanes walks the batch in kTpThreads-wide tiles; lane t of tile b owns sequence
// b + t. Inside a tile the running sums are wave scans joined through one total per wave; between tiles they
// are carried in LDS.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DDL_TP_HD __host__ __device__ __forceinline__
#else
#define DDL_TP_HD inline
#endif

namespace ddl {

constexpr int kTpThreads = 1024;  // lanes of the one workgroup = sequences per tile
constexpr int kTpWave = 64;
constexpr int kTpWaves = kTpThreads / kTpWave;

// tiles of a batch of n sequences (n = 0: none, the loop body never runs)
DDL_TP_HD int64_t tp_tiles(int64_t n) { return n > 0 ? (n + kTpThreads - 1) / kTpThreads : 0; }

// a selected index is dereferenced only inside the corpus; anything else counts as an empty sequence
DDL_TP_HD bool tp_index_ok(int64_t q, int64_t n_corpus) {
  return static_cast<uint64_t>(q) < static_cast<uint64_t>(n_corpus);
}

// length of the sequence [s0, s1) (offsets that decrease -- a corrupt corpus -- give an empty sequence)
DDL_TP_HD int64_t tp_len(int64_t s0, int64_t s1) { return s1 > s0 ? s1 - s0 : 0; }

// segments of a sequence: ceil(len / S), as step 1 of pack_plan_kernel counts them
DDL_TP_HD int64_t tp_seg_count(int64_t len, int64_t S) { return len > 0 ? (len + S - 1) / S : 0; }

// the longest segment a sequence contributes
DDL_TP_HD int64_t tp_seg_max(int64_t len, int64_t S) { return len < S ? len : S; }

// corpus element of the first token of a sequence's j-th segment
DDL_TP_HD int64_t tp_seg_src(int64_t src0, int64_t j, int64_t S) { return src0 + j * S; }

// what precedes a lane's value in the batch: the carry of the earlier tiles + the totals of the earlier waves
// of this tile (wave_tot[kTpWaves]) + the earlier lanes of its wave (incl = the wave's inclusive scan at the lane)
DDL_TP_HD int64_t tp_before(const int64_t* wave_tot, int wv, int64_t carry) {
  int64_t before = carry;
  for (int k = 0; k < wv; ++k) before += wave_tot[k];
  return before;
}
DDL_TP_HD int64_t tp_exclusive(int64_t before, int64_t incl, int64_t v) { return before + incl - v; }

// how many of the segments [first, first + c) lie inside the capacity: only those are written
DDL_TP_HD int64_t tp_seg_writes(int64_t first, int64_t c, int64_t max_segs) {
  int64_t room = max_segs - first;
  if (room < 0) room = 0;
  return c < room ? c : room;
}

}  // namespace ddl
