// Index arithmetic and per-lane routines of the token stream kernels (tokens_stream.hip), shared with host code:
// csrc/kernels/tests/tokens_stream_check.cpp runs them under ASan/UBSan inside a replay of the kernels' loops, in
// which only the wave collectives have a host stand-in.
// Plain inline functions: __host__ __device__ under hipcc, plain under g++ (this header includes nothing of HIP).
//
// The stream of an epoch is concat(document q_0, q_1, ..., q_{n-1}) in the epoch's order; document k occupies
// stream positions [table[k], table[k + 1]), table = the exclusive scan of the lengths (token_stream_table).
// A batch is the window [T0, T1) = rows [row_base, row_base + rows) of S tokens each, cut off at the stream's
// end. token_stream_plan turns it into the pack plan pad_pack_tokens_indexed renders: a segment (a "piece") is
// a maximal run of one document inside one row,
//   seg_offsets[f + j] = piece start - T0          seg_src[f + j] = corpus_offsets[q] + (piece start - table[d])
// numbered by the exclusive scan of the documents' piece counts, and row r = [r * S, (r + 1) * S) clamped to the
// window's tokens. The scans reuse the tile shape of tokens_plan.h: kTpThreads lanes per tile, wave scans joined
// through one total per wave, a carry between tiles.
#pragma once

#include <stdint.h>

#include "tokens_plan.h"

#define DDL_TS_HD DDL_TP_HD

namespace ddl {

// tiles of the table scan over n documents (n = 0: none; table[0] is the middle pass's)
DDL_TS_HD int64_t ts_tiles(int64_t n) { return tp_tiles(n); }

// the window [T0, T1) of rows [row_base, row_base + rows) of a stream of T tokens (T1 < T0: an empty window past
// the end is reported as T1 = T0)
DDL_TS_HD void ts_window(int64_t row_base, int64_t rows, int64_t S, int64_t T, int64_t* T0, int64_t* T1) {
  *T0 = row_base * S;
  const int64_t end = *T0 + rows * S;
  *T1 = end < T ? end : T;
  if (*T1 < *T0) *T1 = *T0;
}

// One step of the wave-wide search for the last d in [lo, hi) with table[d] <= v (table[lo] <= v holds): the 64
// lanes probe lo + lane * step, the entries <= v are a prefix of k >= 1 lanes, and the range narrows to the
// k-th probe's stride. Four steps cover 2^24 + 1 entries.
DDL_TS_HD int64_t ts_search_stride(int64_t lo, int64_t hi) { return (hi - lo + kTpWave - 1) / kTpWave; }
DDL_TS_HD int64_t ts_search_probe(int64_t lo, int64_t stride, int lane) { return lo + lane * stride; }
DDL_TS_HD void ts_search_narrow(int64_t* lo, int64_t* hi, int64_t stride, int k) {
  *lo += (k - 1) * stride;
  if (*lo + stride < *hi) *hi = *lo + stride;
}

// document [a, e) of the stream clipped to the window; returns whether anything is left
DDL_TS_HD bool ts_clip(int64_t a, int64_t e, int64_t T0, int64_t T1, int64_t* lo, int64_t* hi) {
  *lo = a > T0 ? a : T0;
  *hi = e < T1 ? e : T1;
  return *hi > *lo;
}

// pieces of the clipped document [lo, hi), hi > lo: 1 + the row boundaries (multiples of S) strictly inside
DDL_TS_HD int64_t ts_pieces(int64_t lo, int64_t hi, int64_t S) { return 1 + (hi - 1) / S - lo / S; }

// stream position of piece j's first token
DDL_TS_HD int64_t ts_piece_start(int64_t lo, int64_t j, int64_t S) { return j == 0 ? lo : (lo / S + j) * S; }

// the longest piece of [lo, hi): the first (up to its row's end), a whole row in between, the last
DDL_TS_HD int64_t ts_piece_max(int64_t lo, int64_t hi, int64_t S) {
  const int64_t c = ts_pieces(lo, hi, S);
  if (c == 1) return hi - lo;
  if (c > 2) return S;
  const int64_t first = (lo / S + 1) * S - lo, last = hi - ((hi - 1) / S) * S;
  return first > last ? first : last;
}

// The per-lane routines below read memory by a computed index, so kernel and host replay compile the same text.
// order(i) = the corpus document at position i of the order (the kernels: source_row(ri, i)); coffs and table are
// anything indexable by int64 (the kernels: the device pointers; the replay: views that check every index).

// length of document i of an order of n documents (0 past n, and for an index outside the corpus)
template <typename Offs, typename Order>
DDL_TS_HD int64_t ts_doc_len(const Offs& coffs, int64_t n_corpus, const Order& order, int64_t n, int64_t i) {
  if (i >= n) return 0;
  const int64_t q = order(i);
  if (!tp_index_ok(q, n_corpus)) return 0;
  return tp_len(coffs[q], coffs[q + 1]);
}

// One lane of the plan: document d <= d1 of the order clipped to the window [T0, T1). *a = its stream position,
// *lo = where its clipped part starts, *src0 = its first corpus element, *c = its pieces and *mx = the longest.
// *c = *mx = 0, no piece, for a document past d1 or n, outside the corpus or with nothing inside the window.
template <typename Offs, typename Table, typename Order>
DDL_TS_HD void ts_plan_doc(const Offs& coffs, int64_t n_corpus, const Table& table, const Order& order, int64_t n,
                           int64_t d, int64_t d1, int64_t T0, int64_t T1, int64_t S, int64_t* a, int64_t* lo,
                           int64_t* src0, int64_t* c, int64_t* mx) {
  int64_t hi = 0;
  *a = *lo = *src0 = *c = *mx = 0;
  if (d <= d1 && d < n) {  // d1 < n for a table that ends in its total; kept so regardless
    const int64_t q = order(d);
    *a = table[d];
    if (tp_index_ok(q, n_corpus) && ts_clip(*a, table[d + 1], T0, T1, lo, &hi)) {
      *src0 = coffs[q];
      *c = ts_pieces(*lo, hi, S);
      *mx = ts_piece_max(*lo, hi, S);
    }
  }
}

// limits of row r of a window holding n_tok tokens, and its rows with at least one token
DDL_TS_HD int64_t ts_row_limit(int64_t r, int64_t S, int64_t n_tok) { return r * S < n_tok ? r * S : n_tok; }
DDL_TS_HD int64_t ts_rows_used(int64_t n_tok, int64_t S) { return (n_tok + S - 1) / S; }

}  // namespace ddl
