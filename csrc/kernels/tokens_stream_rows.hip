// Token stream loader, shuffled rows: batch row k is stream row rho_k = source_row(rows_ri, k) -- any full row of
// the stream, in any order -- planned on the device by two launches in front of the unchanged
// pad_pack_tokens_indexed (tokens_indexed.hip, pack mode, plan counts read from device memory). The index
// arithmetic is tokens_stream_rows.h; the wave-wide search and reductions are tokens_stream_wave.h.
//
// Where token_stream_plan is one workgroup that walks one contiguous window, every row here is a window of its
// own somewhere in the table: two searches per row, and the rows' segments still numbered row-major into one
// seg_offsets. Both launches are ceil(rows / 16) workgroups of 1024 lanes, one wave per batch row.
//
// token_stream_rows_count (launch A): the wave evaluates rho_k, validates it against table[n], finds the row's
// first and last document by two 64-ary searches of the table and walks the documents between them 64 at a time
// (a loop: arbitrarily many empty documents may lie in between), counting the non-empty clipped ones by ballot /
// popcount and taking the longest. Lane 0 leaves {count or -1, longest, first, last document} in the plan buffer.
// token_stream_rows_write (launch B): every workgroup first reduces the count words of all rows -- the segments in
// front of its own 16 rows, the batch's segments, its invalid rows -- a few thousand int64 out of L2 read once per
// workgroup, in place of a scan launch and of any waiting between workgroups. Each wave then walks its row's
// documents again and writes its segments behind the rows in front; workgroup 0 also writes row_start / row_end,
// seg_offsets[n_seg] and the four counts. An invalid batch writes no segment, only seg_offsets[0] = 0 (the one
// entry the emit kernel reads of a plan whose counts[0] is -1).
// No atomic, no workgroup waits for another, no cooperative launch; every barrier and exit is block-uniform, the
// wave-level loops are wave-uniform.
//
// Bounded reads: table[0 .. n]; corpus_offsets[q] only for 0 <= q < n_corpus (anything else is an empty document;
// corpus_offsets[q + 1] is never needed here, the table holds the lengths); rows_ri.idx[0 .. rows) in mode 1;
// source_row(rows_ri, .) only for positions [rows_ri.base, rows_ri.base + rows), which the launcher checks against
// the Feistel domain, source_row(ri, .) only for documents [0, n); the 4 * rows scratch words. Nothing of the
// corpus itself is read.
// Bounded writes: the scratch words, row_start / row_end [0 .. rows) and counts[0 .. 3] exactly once each;
// seg_offsets[i] / seg_src[i] only for i < max_segs and i < n_seg, seg_offsets[n_seg] only when the batch is valid
// and n_seg <= max_segs, each exactly once; an invalid batch writes seg_offsets[0] once and no other segment entry.
#include "common.h"
#include "launch.h"
#include "tokens_stream_rows.h"
#include "tokens_stream_wave.h"

namespace ddl {
namespace {

__global__ void __launch_bounds__(kTpThreads) token_stream_rows_count_kernel(StreamRowsSpec sp) {
  const int t = threadIdx.x, lane = t & (kTpWave - 1), wv = t / kTpWave;
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kTpWaves + wv;
  if (k < sp.p.rows) {  // wave-uniform; this kernel has no barrier
    const int64_t S = sp.p.seq_len, T = sp.p.table[sp.p.n];
    const int64_t rho = source_row(sp.rows_ri, k);
    const bool valid = tsr_row_valid(rho, T, S);
    int64_t segs = 0, mx = 0, d0 = 0, d1 = 0;
    if (valid) {  // wave-uniform; then T0 < table[n]: both documents exist and are not empty
      const int64_t T0 = rho * S, T1 = T0 + S;
      d0 = ts_wave_last_le(sp.p.table, sp.p.n + 1, T0);
      d1 = ts_wave_last_le(sp.p.table, sp.p.n + 1, T1 - 1);
      for (int64_t b = d0; b <= d1; b += kTpWave) {  // wave-uniform trip count
        int64_t q, a, lo = 0, hi = 0;
        const bool has =
            tsr_doc(sp.p.table, sp.p.n_corpus, TsOrder{sp.p.ri}, sp.p.n, b + lane, d1, T0, T1, &q, &a, &lo, &hi);
        segs += __popcll(__ballot(has));
        if (has && hi - lo > mx) mx = hi - lo;
      }
      mx = ts_wave_max(mx);
    }
    if (lane == 0) {
      int64_t* w = sp.scratch + k;
      w[0] = tsr_count_word(valid, segs);
      w[sp.p.rows] = mx;
      w[2 * sp.p.rows] = d0;
      w[3 * sp.p.rows] = d1;
    }
  }
}

__global__ void __launch_bounds__(kTpThreads) token_stream_rows_write_kernel(StreamRowsSpec sp) {
  __shared__ int64_t wave_before[kTpWaves], wave_total[kTpWaves], wave_bad[kTpWaves], wave_max[kTpWaves];
  const int t = threadIdx.x, lane = t & (kTpWave - 1), wv = t / kTpWave;
  const int64_t S = sp.p.seq_len, rows = sp.p.rows;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kTpWaves;
  const int64_t* cnt = sp.scratch;
  const bool lead = blockIdx.x == 0;  // block-uniform: the workgroup that writes the rows' limits and the counts
  int64_t before = 0, total = 0, bad = 0, mx = 0;
  for (int64_t r = t; r < rows; r += kTpThreads) {
    const int64_t w = cnt[r], c = tsr_count_segs(w);
    total += c;
    if (r < row0) before += c;
    bad += tsr_count_invalid(w);
    if (lead) {
      const int64_t m = cnt[rows + r];
      mx = m > mx ? m : mx;
    }
  }
  before = ts_wave_incl_scan(before);
  total = ts_wave_incl_scan(total);
  bad = ts_wave_incl_scan(bad);
  mx = ts_wave_max(mx);
  if (lane == kTpWave - 1) {
    wave_before[wv] = before;
    wave_total[wv] = total;
    wave_bad[wv] = bad;
    wave_max[wv] = mx;
  }
  __syncthreads();
  const int64_t n_seg = tp_before(wave_total, kTpWaves, 0);
  const int64_t n_bad = tp_before(wave_bad, kTpWaves, 0);  // block-uniform
  const int64_t k = row0 + wv;
  if (k < rows && n_bad == 0) {  // wave-uniform
    int64_t first = tp_before(wave_before, kTpWaves, 0);
    for (int64_t j = row0; j < k; ++j) first += tsr_count_segs(cnt[j]);  // the rows of this workgroup in front
    const int64_t rho = source_row(sp.rows_ri, k);
    const int64_t T0 = rho * S, T1 = T0 + S;
    const int64_t d0 = cnt[2 * rows + k], d1 = cnt[3 * rows + k];
    for (int64_t b = d0; b <= d1; b += kTpWave) {  // wave-uniform trip count
      int64_t q, a, lo = 0, hi = 0;
      const bool has =
          tsr_doc(sp.p.table, sp.p.n_corpus, TsOrder{sp.p.ri}, sp.p.n, b + lane, d1, T0, T1, &q, &a, &lo, &hi);
      const unsigned long long votes = __ballot(has);
      if (has) {
        const int64_t i = first + __popcll(votes & ((1ull << lane) - 1ull));
        if (tp_seg_writes(i, 1, sp.p.max_segs) > 0) {
          sp.p.seg_offsets[i] = tsr_seg_offset(k, rho, S, lo);
          sp.p.seg_src[i] = tsr_seg_src(sp.p.corpus_offsets[q], a, lo);
        }
      }
      first += __popcll(votes);
    }
  }
  if (lead) {
    for (int64_t r = t; r < rows; r += kTpThreads) {
      sp.p.row_start[r] = r * S;
      sp.p.row_end[r] = (r + 1) * S;
    }
    if (t == 0) {
      int64_t m = 0;
      for (int w = 0; w < kTpWaves; ++w) m = wave_max[w] > m ? wave_max[w] : m;
      const bool ok = tsr_batch_ok(n_bad, n_seg, sp.p.max_segs);
      const int64_t n_tok = tsr_batch_tokens(rows, n_bad, S);
      if (ok) sp.p.seg_offsets[n_seg] = n_tok;
      if (n_bad != 0) sp.p.seg_offsets[0] = 0;  // no segment was written: the entry a plan with counts[0] = -1 shows
      sp.p.counts[0] = ok ? rows : -1;
      sp.p.counts[1] = n_seg;
      sp.p.counts[2] = n_tok;
      sp.p.counts[3] = m;
    }
  }
}

}  // namespace

int token_stream_plan_rows(const StreamRowsSpec& spec, hipStream_t st) {
  if (!ts_plan_args_ok(spec.p) || spec.stream_rows < 0 || !spec.scratch) return -2;
  if (spec.stream_rows > INT64_MAX / spec.p.seq_len) return -2;
  if (!row_index_ok(spec.rows_ri, spec.p.rows)) return -2;
  if (spec.rows_ri.mode == 2) {  // a permutation of the stream's rows, asked for positions inside it
    if (spec.rows_ri.keys.n != static_cast<uint64_t>(spec.stream_rows)) return -2;
    if (spec.rows_ri.base > spec.stream_rows - spec.p.rows) return -2;
  }
  const dim3 grid(static_cast<uint32_t>(tsr_blocks(spec.p.rows))), block(kTpThreads);
  hipLaunchKernelGGL(token_stream_rows_count_kernel, grid, block, 0, st, spec);
  hipLaunchKernelGGL(token_stream_rows_write_kernel, grid, block, 0, st, spec);
  return static_cast<int>(hipGetLastError());
}

}  // namespace ddl
