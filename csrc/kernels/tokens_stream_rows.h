// Index arithmetic and the per-lane routine of the shuffled-row plan of the token stream (tokens_stream_rows.hip),
// shared with host code: csrc/kernels/tests/tokens_stream_rows_check.cpp runs them under ASan/UBSan inside a replay
// of both launches' per-wave loops, in which only the wave collectives have a host stand-in.
// Plain inline functions: __host__ __device__ under hipcc, plain under g++ (this header includes nothing of HIP).
//
// Batch row k is stream row rho_k (any row of the stream, in any order, repeats allowed): the window
// [rho_k * S, (rho_k + 1) * S) of the table of tokens_stream.h. A row is valid when it is a full row of the
// stream, 0 <= rho_k and (rho_k + 1) * S <= T = table[n]; one invalid row makes the batch invalid. Inside one row
// a document makes at most one segment, so a row's segments are its non-empty clipped documents, in order:
//   seg_offsets[f_k + j] = k * S + (lo - rho_k * S)        seg_src[f_k + j] = corpus_offsets[q] + (lo - table[d])
// lo = max(table[d], rho_k * S), f_k = the segments of the valid rows in front of row k. Launch A leaves four
// words per row in the plan buffer (kTsrRowWords arrays of `rows` int64: segment count or -1 for an invalid row,
// longest segment, first and last document); launch B reduces them per workgroup and writes the plan.
#pragma once

#include <stdint.h>

#include "tokens_stream.h"

#define DDL_TSR_HD DDL_TS_HD

namespace ddl {

constexpr int kTsrRowWords = 4;  // per-row int64 arrays between the launches: count, longest, first, last document

// workgroups of either launch: one wave per batch row, kTpWaves rows per workgroup
DDL_TSR_HD int64_t tsr_blocks(int64_t rows) { return (rows + kTpWaves - 1) / kTpWaves; }
DDL_TSR_HD int64_t tsr_scratch_words(int64_t rows) { return kTsrRowWords * rows; }

// full rows of a stream of T tokens; a selected row is valid inside [0, that)
DDL_TSR_HD int64_t tsr_stream_rows(int64_t T, int64_t S) { return T > 0 ? T / S : 0; }
DDL_TSR_HD bool tsr_row_valid(int64_t rho, int64_t T, int64_t S) { return rho >= 0 && rho < tsr_stream_rows(T, S); }

// One lane of either launch: document d of the order clipped to the row [T0, T1), whether anything is left (d past
// d1, outside [0, n) or with an index outside the corpus: nothing). table and order as for ts_plan_doc.
template <typename Table, typename Order>
DDL_TSR_HD bool tsr_doc(const Table& table, int64_t n_corpus, const Order& order, int64_t n, int64_t d, int64_t d1,
                        int64_t T0, int64_t T1, int64_t* q, int64_t* a, int64_t* lo, int64_t* hi) {
  if (d > d1 || d < 0 || d >= n) return false;
  *q = order(d);
  *a = table[d];
  return tp_index_ok(*q, n_corpus) && ts_clip(*a, table[d + 1], T0, T1, lo, hi);
}

// a row's count word: its segments, or -1 for an invalid row (which adds nothing to the batch)
DDL_TSR_HD int64_t tsr_count_word(bool valid, int64_t segs) { return valid ? segs : -1; }
DDL_TSR_HD int64_t tsr_count_segs(int64_t word) { return word > 0 ? word : 0; }
DDL_TSR_HD int64_t tsr_count_invalid(int64_t word) { return word < 0 ? 1 : 0; }

// batch-local start of the segment whose first stream position is lo, in batch row k = stream row rho
DDL_TSR_HD int64_t tsr_seg_offset(int64_t k, int64_t rho, int64_t S, int64_t lo) { return k * S + (lo - rho * S); }
// corpus element of that segment's first token: document [a, ...) of the stream starts at corpus element src0
DDL_TSR_HD int64_t tsr_seg_src(int64_t src0, int64_t a, int64_t lo) { return src0 + (lo - a); }

// the four counts of the batch: {rows or -1, segments, tokens, longest segment}, segments / tokens / longest over
// the valid rows only
DDL_TSR_HD bool tsr_batch_ok(int64_t n_invalid, int64_t n_seg, int64_t max_segs) {
  return n_invalid == 0 && n_seg <= max_segs;
}
DDL_TSR_HD int64_t tsr_batch_tokens(int64_t rows, int64_t n_invalid, int64_t S) { return (rows - n_invalid) * S; }

}  // namespace ddl
