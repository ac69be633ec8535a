// Host check of the shuffled-row plan kernels' index arithmetic (csrc/kernels/tokens_stream_rows.h), built with
// -fsanitize=address,undefined by tests/test_token_stream_rows.py. It replays both launches of
// tokens_stream_rows.hip workgroup by workgroup, wave by wave, lane by lane on the host: the corpus offsets, the
// order, the table, the row index, the per-row scratch and every plan array are heap buffers of exactly their
// size, so an offset read for an index outside the corpus, a probe past the table or a segment written past the
// capacity is a heap overflow. Every write index is checked against the sizes as well, every output element must
// be written exactly once, and the results are compared with a plain serial construction, token by token. A
// lane's document clipped to its row is the kernels' source (tsr_doc), reading through views that name an index
// outside a buffer. Only the wave collectives are stood in for: the ballot of a step is the set of the wave's lanes
// whose document leaves something in the row; a wave sum is the serial sum of the wave's 64 lanes.
#include "../tokens_stream_rows.h"
#include "stream_check_common.h"

namespace {

void run_plan(const char* name, const Corpus& c, const std::vector<int64_t>& rho_in, int64_t S, int64_t max_segs) {
  ++g_cases;
  const int64_t rows = static_cast<int64_t>(rho_in.size()), n = c.n, T = c.table[n];
  const View table = c.table_view(), order = c.order_view();
  int64_t* rho = exact<int64_t>(rows);  // rows_ri.idx
  for (int64_t k = 0; k < rows; ++k) rho[k] = rho_in[k];
  int64_t* scratch = exact<int64_t>(ddl::tsr_scratch_words(rows));
  int64_t* seg_offsets = exact<int64_t>(max_segs + 1);
  int64_t* seg_src = exact<int64_t>(max_segs);
  int64_t* row_start = exact<int64_t>(rows);
  int64_t* row_end = exact<int64_t>(rows);
  int64_t counts[4] = {-77, -77, -77, -77};
  std::vector<int> w_scr(ddl::tsr_scratch_words(rows), 0), w_so(max_segs + 1, 0), w_ss(max_segs, 0), w_row(rows, 0);
  const int64_t blocks = ddl::tsr_blocks(rows);
  if (blocks * ddl::kTpWaves < rows || (blocks - 1) * ddl::kTpWaves >= rows) fail(name, "grid does not cover the rows");

  // ---- launch A, one wave per row
  for (int64_t blk = 0; blk < blocks; ++blk) {
    for (int wv = 0; wv < ddl::kTpWaves; ++wv) {
      const int64_t k = blk * ddl::kTpWaves + wv;
      if (k >= rows) continue;
      const int64_t r = rho[k];
      const bool valid = ddl::tsr_row_valid(r, T, S);
      int64_t segs = 0, mx = 0, d0 = 0, d1 = 0;
      if (valid) {
        const int64_t T0 = r * S, T1 = T0 + S;
        d0 = replay_search(name, c.table, n + 1, T0);
        d1 = replay_search(name, c.table, n + 1, T1 - 1);
        if (!(c.table[d0] <= T0 && T0 < c.table[d0 + 1] && c.table[d1] <= T1 - 1 && T1 - 1 < c.table[d1 + 1]))
          fail(name, "search result");
        for (int64_t b = d0; b <= d1; b += ddl::kTpWave) {
          for (int lane = 0; lane < ddl::kTpWave; ++lane) {
            int64_t q, a, lo = 0, hi = 0;
            if (ddl::tsr_doc(table, c.n_corpus, order, n, b + lane, d1, T0, T1, &q, &a, &lo, &hi)) {
              ++segs;
              if (hi - lo > mx) mx = hi - lo;
            }
          }
        }
      }
      const int64_t words[ddl::kTsrRowWords] = {ddl::tsr_count_word(valid, segs), mx, d0, d1};
      for (int w = 0; w < ddl::kTsrRowWords; ++w) {
        scratch[w * rows + k] = words[w];
        ++w_scr[w * rows + k];
      }
    }
  }
  for (int v : w_scr)
    if (v != 1) fail(name, "scratch word not written exactly once");

  // ---- launch B
  for (int64_t blk = 0; blk < blocks; ++blk) {
    const int64_t row0 = blk * ddl::kTpWaves;
    const bool lead = blk == 0;
    int64_t wave_before[ddl::kTpWaves] = {}, wave_total[ddl::kTpWaves] = {}, wave_bad[ddl::kTpWaves] = {},
            wave_max[ddl::kTpWaves] = {};
    for (int t = 0; t < ddl::kTpThreads; ++t) {  // the lanes' strided sums, joined per wave
      int64_t before = 0, total = 0, bad = 0, mx = 0;
      for (int64_t r = t; r < rows; r += ddl::kTpThreads) {
        const int64_t w = scratch[r], cc = ddl::tsr_count_segs(w);
        total += cc;
        if (r < row0) before += cc;
        bad += ddl::tsr_count_invalid(w);
        if (lead && scratch[rows + r] > mx) mx = scratch[rows + r];
      }
      const int wv = t / ddl::kTpWave;
      wave_before[wv] += before, wave_total[wv] += total, wave_bad[wv] += bad;
      if (mx > wave_max[wv]) wave_max[wv] = mx;
    }
    const int64_t n_seg = ddl::tp_before(wave_total, ddl::kTpWaves, 0);
    const int64_t n_bad = ddl::tp_before(wave_bad, ddl::kTpWaves, 0);
    for (int wv = 0; wv < ddl::kTpWaves; ++wv) {
      const int64_t k = row0 + wv;
      if (!(k < rows && n_bad == 0)) continue;
      int64_t first = ddl::tp_before(wave_before, ddl::kTpWaves, 0);
      for (int64_t j = row0; j < k; ++j) first += ddl::tsr_count_segs(scratch[j]);
      const int64_t r = rho[k], T0 = r * S, T1 = T0 + S;
      const int64_t d0 = scratch[2 * rows + k], d1 = scratch[3 * rows + k];
      for (int64_t b = d0; b <= d1; b += ddl::kTpWave) {
        int votes = 0;
        for (int lane = 0; lane < ddl::kTpWave; ++lane) {  // votes so far = the ballot's bits below the lane
          int64_t q, a, lo = 0, hi = 0;
          if (!ddl::tsr_doc(table, c.n_corpus, order, n, b + lane, d1, T0, T1, &q, &a, &lo, &hi)) continue;
          const int64_t i = first + votes++;
          if (ddl::tp_seg_writes(i, 1, max_segs) > 0) {
            if (i < 0 || i >= max_segs) {
              fail(name, "segment written past the capacity");
              continue;
            }
            if (q < 0 || q >= c.n_corpus) fail(name, "corpus offsets read out of range");
            seg_offsets[i] = ddl::tsr_seg_offset(k, r, S, lo);
            seg_src[i] = ddl::tsr_seg_src(c.coffs[q], a, lo);
            ++w_so[i], ++w_ss[i];
          }
        }
        first += votes;
      }
    }
    if (lead) {
      for (int64_t r = 0; r < rows; ++r) {
        row_start[r] = r * S, row_end[r] = (r + 1) * S;
        ++w_row[r];
      }
      int64_t m = 0;
      for (int w = 0; w < ddl::kTpWaves; ++w) m = wave_max[w] > m ? wave_max[w] : m;
      const bool ok = ddl::tsr_batch_ok(n_bad, n_seg, max_segs);
      const int64_t n_tok = ddl::tsr_batch_tokens(rows, n_bad, S);
      if (ok) {
        seg_offsets[n_seg] = n_tok;
        ++w_so[n_seg];
      }
      if (n_bad != 0) {
        seg_offsets[0] = 0;
        ++w_so[0];
      }
      counts[0] = ok ? rows : -1;
      counts[1] = n_seg, counts[2] = n_tok, counts[3] = m;
    }
  }

  // ---- the plain serial construction, token by token over the valid rows
  bool ok = true;
  int64_t seg = 0, mx = 0, n_valid = 0;
  bool all_valid = true;
  for (int64_t k = 0; k < rows; ++k)
    if (!(rho[k] >= 0 && rho[k] <= T / S - 1)) all_valid = false;
  for (int64_t k = 0; k < rows; ++k) {
    if (!(rho[k] >= 0 && rho[k] <= T / S - 1)) continue;
    ++n_valid;
    int64_t d = 0, prev_d = -1, run = 0;
    for (int64_t g = rho[k] * S; g < (rho[k] + 1) * S; ++g) {
      while (c.table[d + 1] <= g) ++d;  // the document holding g (empty ones are skipped)
      if (d != prev_d) {  // a new piece (the row's first token included)
        if (all_valid && seg < max_segs) {
          const int64_t q = c.order[d];
          ok = ok && w_so[seg] == 1 && w_ss[seg] == 1 && seg_offsets[seg] == k * S + (g - rho[k] * S) &&
               seg_src[seg] == c.coffs[q] + (g - c.table[d]);
        }
        ++seg;
        run = 0;
        prev_d = d;
      }
      ++run;
      mx = run > mx ? run : mx;
    }
  }
  ok = ok && counts[1] == seg && counts[2] == n_valid * S && counts[3] == mx;
  if (!all_valid) {  // no segment entry but the first
    ok = ok && counts[0] == -1 && w_so[0] == 1 && seg_offsets[0] == 0;
    for (int64_t i = 1; i <= max_segs; ++i) ok = ok && w_so[i] == 0;
    for (int64_t i = 0; i < max_segs; ++i) ok = ok && w_ss[i] == 0;
  } else if (seg <= max_segs) {
    ok = ok && counts[0] == rows && w_so[seg] == 1 && seg_offsets[seg] == rows * S;
    for (int64_t i = seg + 1; i <= max_segs; ++i) ok = ok && w_so[i] == 0;
    for (int64_t i = seg; i < max_segs; ++i) ok = ok && w_ss[i] == 0;
  } else {
    ok = ok && counts[0] == -1 && w_so[max_segs] == 0 && seg_offsets[0] == 0;
  }
  for (int64_t r = 0; r < rows; ++r) ok = ok && w_row[r] == 1 && row_start[r] == r * S && row_end[r] == (r + 1) * S;
  if (!ok) {
    printf("%s (n %lld, rows %lld, S %lld, max_segs %lld): plan mismatch\n", name, (long long)n, (long long)rows,
           (long long)S, (long long)max_segs);
    ++g_failures;
  }
  for (void* p : {(void*)rho, (void*)scratch, (void*)seg_offsets, (void*)seg_src, (void*)row_start, (void*)row_end})
    free(p);
}

// lens: the corpus; order: the documents of the stream (in range). Runs the plan over selections of every kind at
// capacities that fit and that do not.
void run_case(const char* name, const std::vector<int64_t>& lens, const std::vector<int64_t>& order) {
  ++g_cases;
  Corpus c = make_corpus(name, lens, order);
  serial_table(&c);
  const int64_t T = c.table[c.n];
  Lcg rng{0x9E3779B97F4A7C15ull + static_cast<uint64_t>(T)};
  for (int64_t S : {1, 4, 6, 37, 512}) {
    const int64_t full = T / S;
    for (int64_t rows : {1, 3, 16, 17, 40}) {
      std::vector<int64_t> ident, rev, rnd, rep, bad_neg, bad_tail, bad_far;
      for (int64_t k = 0; k < rows; ++k) {
        ident.push_back(full ? k % full : 0);
        rev.push_back(full ? full - 1 - k % full : 0);
        rnd.push_back(full ? rng.next() % full : 0);
        rep.push_back(full ? rnd[0] : 0);
      }
      bad_neg = bad_tail = bad_far = rnd;
      bad_neg[rows / 2] = -1;
      bad_tail[rows - 1] = full;  // the partial last row, or the first row past the end
      bad_far[0] = INT64_MAX / S;
      const int64_t safe = rows * S;  // a segment holds a token
      std::vector<std::vector<int64_t>> sels = {bad_neg, bad_tail, bad_far};
      if (full) sels.insert(sels.end(), {ident, rev, rnd, rep});
      for (const auto& sel : sels) {
        run_plan(name, c, sel, S, safe);
        run_plan(name, c, sel, S, 1);
        run_plan(name, c, sel, S, rows + 1);
      }
    }
  }
  free_corpus(&c);
}

void run_all() {
  const std::vector<int64_t> lens13 = mod_lens(3001, 13), lens41 = mod_lens(3001, 41), ones = mod_lens(3001, 2, 1);
  for (int64_t n : {1, 63, 64, 65, 1025, 3001}) {
    const std::vector<int64_t> order = stride_order(n, 7, 5, 3001);
    run_case("i % 13", lens13, order);
    run_case("i % 41", lens41, order);
    run_case("1-2 tokens", ones, order);  // hundreds of documents per row at S = 512: several steps of the walk
  }
  run_case("all empty", std::vector<int64_t>(50, 0), mod_lens(1100, 50));  // no full row: every selection is invalid
  std::vector<int64_t> gap = {3};  // a run of 200 empty documents between two documents of one row
  for (int i = 0; i < 200; ++i) gap.push_back(0);
  gap.push_back(9);
  for (int i = 0; i < 70; ++i) gap.push_back(0);
  gap.push_back(4);
  std::vector<int64_t> gap_order;
  for (size_t i = 0; i < gap.size(); ++i) gap_order.push_back(static_cast<int64_t>(i));
  run_case("empty runs", gap, gap_order);
  std::vector<int64_t> longs = {5000, 0, 4096, 4097, 1};  // rows wholly inside one document
  run_case("long documents", longs, {3, 1, 0, 4, 2});
  // more rows than one pass of the 1024 lanes of the reduction
  Corpus c = make_corpus("1025 rows", lens13, stride_order(3001, 11, 3, 3001));
  serial_table(&c);
  std::vector<int64_t> many = stride_order(1025, 37, 0, c.table[3001] / 8);
  run_plan("1025 rows", c, many, 8, 1025 * 8);
  run_plan("1025 rows", c, many, 8, 1500);
  many[1024] = -5;
  run_plan("1025 rows, the last invalid", c, many, 8, 1025 * 8);
  free_corpus(&c);
}

// Far corpus: eight documents of 2^40 tokens among short and empty ones, one of 2^32 + 3, so that the corpus
// offsets, the table and every seg_src pass 2^32 and 2^40 and reach 2^43. Nothing of that size is materialised.
std::vector<int64_t> far_lens() {
  const int64_t big = int64_t{1} << 40;
  return {5, big, 0, 7, big, big, 1, (int64_t{1} << 32) + 3, big, 0, 0, big, 4097, big, big, 3, big, 11};
}

void run_far() {
  const std::vector<int64_t> lens = far_lens();
  const std::vector<int64_t> order = {16, 3, 1, 9, 7, 0, 13, 2, 4, 17, 5, 12, 8, 6, 11, 10, 14, 15};
  ++g_cases;
  Corpus c = make_corpus("far", lens, order);
  serial_table(&c);
  const int64_t T = c.table[c.n];
  if (T <= (int64_t{1} << 43)) fail("far", "the stream is not far");
  for (int64_t S : {6, 37, 512}) {
    const int64_t full = T / S;
    std::vector<int64_t> sel = {0, full - 1, (int64_t{1} << 31) / S, (int64_t{1} << 32) / S, (int64_t{1} << 32) / S + 1,
                                (int64_t{1} << 40) / S, (int64_t{1} << 43) / S};
    for (int64_t i = 1; i < c.n; ++i)  // the rows on both sides of, and across, every document border
      for (int64_t d : {-1, 0, 1}) sel.push_back(c.table[i] / S + d);
    for (int64_t& r : sel) r = r < 0 ? 0 : (r > full - 1 ? full - 1 : r);
    const int64_t rows = static_cast<int64_t>(sel.size());
    run_plan("far", c, sel, S, rows * S);
    run_plan("far", c, sel, S, rows + 1);
    std::vector<int64_t> bad = sel;
    bad[3] = full;  // the first row past the full rows
    run_plan("far, one invalid", c, bad, S, rows * S);
  }
  free_corpus(&c);
}

}  // namespace

int main() {
  run_all();
  run_far();
  return finish("tokens stream rows check");
}
