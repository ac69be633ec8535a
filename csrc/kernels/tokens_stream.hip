// Token stream loader: "concatenate the epoch's shuffled documents and cut every S tokens", planned on the
// device. Two kernels in front of the unchanged pad_pack_tokens_indexed (tokens_indexed.hip, pack mode, plan
// counts read from device memory); all the index arithmetic is tokens_stream.h.
//
// token_stream_table, once per epoch: table[i] = the tokens in front of document i of the epoch's order, a
// device-wide exclusive scan over all n documents as three plain launches on one stream -- (1) one workgroup per
// 1024-document tile sums its lengths, (2) one workgroup scans the tile totals in place, carried from 1024 to
// 1024 tiles as token_batch_descriptor_kernel carries its sums, and writes table[n], (3) one workgroup per tile
// scans its lengths again behind its tile's sum and writes table. Passes 1 and 3 evaluate source_row (the Feistel
// permutation inline, or the identity) and read two corpus offsets per document: 16 B read and 8 B written per
// document and pass, no n-sized index anywhere. No atomic, no workgroup waits for another, no cooperative launch;
// every barrier and exit is block-uniform.
//
// token_stream_plan, once per batch, one workgroup shaped like token_batch_descriptor_kernel: the window's first
// and last document by a wave-wide 64-ary search of the table (4 dependent loads for 2^24 documents, where a
// binary search has 24), then the documents in 1024-wide tiles: a lane clips its document to the window, counts
// its pieces, takes part in the wave scan of the counts and writes its pieces' seg_offsets / seg_src.
//
// Bounded reads: corpus_offsets[q] and corpus_offsets[q + 1] only for 0 <= q < n_corpus (anything else is an
// empty document); table[0 .. n]; source_row only for positions [ri.base, ri.base + n), which the launcher
// checks against the Feistel domain. Nothing of the corpus itself is read.
// Bounded writes: table[0 .. n] and tile_sums[0 .. tiles) exactly once each (tile_sums once per pass 1 and once
// per pass 2). The plan writes seg_offsets[k] / seg_src[k] only for k < max_segs, seg_offsets[n_seg] only when
// n_seg <= max_segs, row_start / row_end [0 .. rows) and counts[0 .. 3], each exactly once.
#include "common.h"
#include "launch.h"
#include "tokens_stream.h"
#include "tokens_stream_wave.h"

namespace ddl {
namespace {

// pass 1: tile_sums[tile] = the tokens of the tile's documents
__global__ void __launch_bounds__(kTpThreads) token_stream_tile_sums_kernel(StreamTableSpec sp) {
  __shared__ int64_t wave_tot[kTpWaves];
  const int t = threadIdx.x, lane = t & (kTpWave - 1), wv = t / kTpWave;
  const int64_t tile = blockIdx.x;
  const int64_t len = ts_doc_len(sp.corpus_offsets, sp.n_corpus, TsOrder{sp.ri}, sp.n, tile * kTpThreads + t);
  const int64_t incl = ts_wave_incl_scan(len);
  if (lane == kTpWave - 1) wave_tot[wv] = incl;
  __syncthreads();
  if (t == 0) sp.tile_sums[tile] = tp_before(wave_tot, kTpWaves, 0);
}

// pass 2: tile_sums -> its exclusive scan, in place; table[n] = the stream's length
__global__ void __launch_bounds__(kTpThreads) token_stream_tile_scan_kernel(StreamTableSpec sp, int64_t tiles) {
  __shared__ int64_t wave_tot[kTpWaves];
  __shared__ int64_t carry;
  const int t = threadIdx.x, lane = t & (kTpWave - 1), wv = t / kTpWave;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int64_t b = 0; b < tiles; b += kTpThreads) {  // block-uniform trip count
    const int64_t i = b + t;
    const int64_t v = i < tiles ? sp.tile_sums[i] : 0;
    const int64_t incl = ts_wave_incl_scan(v);
    if (lane == kTpWave - 1) wave_tot[wv] = incl;
    __syncthreads();
    const int64_t before = tp_before(wave_tot, wv, carry);
    if (i < tiles) sp.tile_sums[i] = tp_exclusive(before, incl, v);
    __syncthreads();  // every lane has read the carry and the wave totals
    if (t == kTpThreads - 1) carry = before + incl;
    __syncthreads();
  }
  if (t == 0) sp.table[sp.n] = carry;
}

// pass 3: table[i] = tile_sums[tile] + the tokens of the tile's documents in front of i
__global__ void __launch_bounds__(kTpThreads) token_stream_tile_write_kernel(StreamTableSpec sp) {
  __shared__ int64_t wave_tot[kTpWaves];
  const int t = threadIdx.x, lane = t & (kTpWave - 1), wv = t / kTpWave;
  const int64_t tile = blockIdx.x;
  const int64_t i = tile * kTpThreads + t;
  const int64_t len = ts_doc_len(sp.corpus_offsets, sp.n_corpus, TsOrder{sp.ri}, sp.n, i);
  const int64_t incl = ts_wave_incl_scan(len);
  if (lane == kTpWave - 1) wave_tot[wv] = incl;
  __syncthreads();
  if (i < sp.n) sp.table[i] = tp_exclusive(tp_before(wave_tot, wv, sp.tile_sums[tile]), incl, len);
}

// The plan kernel's argument: StreamPlanSpec with row_base between n and rows. With row_base behind the shared block,
// the layout the host-side spec has, `counts` leaves the argument's last eight bytes and the kernel measured 3 us (6%)
// slower at 2048 rows, so the launcher passes the fields in this order.
struct StreamPlanArgs {
  const int64_t* table;
  const int64_t* corpus_offsets;
  int64_t n_corpus;
  RowIndex ri;
  int64_t n, row_base, rows, seq_len, max_segs;
  int64_t *seg_offsets, *seg_src, *row_start, *row_end, *counts;
};

__global__ void __launch_bounds__(kTpThreads) token_stream_plan_kernel(StreamPlanArgs sp) {
  __shared__ int64_t wave_seg[kTpWaves], wave_max[kTpWaves];
  __shared__ int64_t carry_seg, carry_max;
  const int t = threadIdx.x, lane = t & (kTpWave - 1), wv = t / kTpWave;
  const int64_t S = sp.seq_len;
  int64_t T0, T1;
  ts_window(sp.row_base, sp.rows, S, sp.table[sp.n], &T0, &T1);  // block-uniform
  const int64_t n_tok = T1 - T0;
  if (t == 0) carry_seg = carry_max = 0;
  __syncthreads();
  if (n_tok > 0) {  // block-uniform; then T0 < table[n]: both documents exist and are not empty
    const int64_t d0 = ts_wave_last_le(sp.table, sp.n + 1, T0);
    const int64_t d1 = ts_wave_last_le(sp.table, sp.n + 1, T1 - 1);
    for (int64_t b = d0; b <= d1; b += kTpThreads) {  // block-uniform trip count
      const int64_t d = b + t;
      int64_t a, lo, src0, c, mx;
      ts_plan_doc(sp.corpus_offsets, sp.n_corpus, sp.table, TsOrder{sp.ri}, sp.n, d, d1, T0, T1, S, &a,
                  &lo, &src0, &c, &mx);
      const int64_t incl = ts_wave_incl_scan(c);
      mx = ts_wave_max(mx);
      if (lane == kTpWave - 1) {
        wave_seg[wv] = incl;
        wave_max[wv] = mx;
      }
      __syncthreads();
      const int64_t before = tp_before(wave_seg, wv, carry_seg);
      const int64_t first = tp_exclusive(before, incl, c);
      const int64_t cnt = tp_seg_writes(first, c, sp.max_segs);
      for (int64_t j = 0; j < cnt; ++j) {
        const int64_t p = ts_piece_start(lo, j, S);
        sp.seg_offsets[first + j] = p - T0;
        sp.seg_src[first + j] = src0 + (p - a);
      }
      __syncthreads();  // every lane has read the carry and the wave totals
      if (t == kTpThreads - 1) carry_seg = before + incl;
      if (t == 0) {
        int64_t m = carry_max;
        for (int k = 0; k < kTpWaves; ++k) m = wave_max[k] > m ? wave_max[k] : m;
        carry_max = m;
      }
      __syncthreads();
    }
  }
  for (int64_t r = t; r < sp.rows; r += kTpThreads) {
    sp.row_start[r] = ts_row_limit(r, S, n_tok);
    sp.row_end[r] = ts_row_limit(r + 1, S, n_tok);
  }
  if (t == 0) {
    const int64_t n_seg = carry_seg;
    const bool fits = n_seg <= sp.max_segs;
    if (fits) sp.seg_offsets[n_seg] = n_tok;  // n_seg = 0: the only entry; an overflowed plan keeps entry 0 = 0
    sp.counts[0] = fits ? ts_rows_used(n_tok, S) : -1;
    sp.counts[1] = n_seg;
    sp.counts[2] = n_tok;
    sp.counts[3] = carry_max;
  }
}

}  // namespace

int64_t token_stream_table_scratch(int64_t n) { return ts_tiles(n) > 0 ? ts_tiles(n) : 1; }

int token_stream_table(const StreamTableSpec& spec, hipStream_t st) {
  if (spec.n < 0 || spec.n_corpus < 0 || !spec.table || !spec.tile_sums) return -2;
  if (spec.n_corpus > 0 && !spec.corpus_offsets) return -2;
  if (!row_index_ok(spec.ri, spec.n)) return -2;
  const int64_t tiles = ts_tiles(spec.n);
  if (tiles > 0x7FFFFFFF) return -4;
  const dim3 grid(static_cast<uint32_t>(tiles)), block(kTpThreads);
  if (tiles > 0) hipLaunchKernelGGL(token_stream_tile_sums_kernel, grid, block, 0, st, spec);
  hipLaunchKernelGGL(token_stream_tile_scan_kernel, dim3(1), block, 0, st, spec, tiles);
  if (tiles > 0) hipLaunchKernelGGL(token_stream_tile_write_kernel, grid, block, 0, st, spec);
  return static_cast<int>(hipGetLastError());
}

int token_stream_plan(const StreamPlanSpec& spec, hipStream_t st) {
  if (!ts_plan_args_ok(spec.p) || spec.row_base < 0) return -2;
  if (spec.row_base > (INT64_MAX / spec.p.seq_len) - spec.p.rows) return -2;  // (row_base + rows) * S fits int64
  const StreamPlanOut& p = spec.p;
  const StreamPlanArgs args{p.table,    p.corpus_offsets, p.n_corpus, p.ri,          p.n,       spec.row_base,
                            p.rows,     p.seq_len,        p.max_segs, p.seg_offsets, p.seg_src, p.row_start,
                            p.row_end,  p.counts};
  hipLaunchKernelGGL(token_stream_plan_kernel, dim3(1), dim3(kTpThreads), 0, st, args);
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
