// Host check of the token stream kernels' index arithmetic (csrc/kernels/tokens_stream.h), built with
// -fsanitize=address,undefined by tests/test_token_stream.py. It replays the kernels' loops (tokens_stream.hip)
// tile by tile, wave by wave, lane by lane on the host: the corpus offsets, the order, the table, the tile sums
// and every plan array are heap buffers of exactly their size, so an offset read for an index outside the corpus,
// a probe past the table or a segment written past the capacity is a heap overflow. Every write index is checked
// against the sizes as well, every output element must be written exactly once, and the results are compared
// with plain serial loops. A lane's own work -- its document's length, its document clipped to the window and
// counted -- is the kernels' source (ts_doc_len, ts_plan_doc), reading through views that name an index outside a
// buffer. Only the wave collectives are stood in for: the wave scan is the serial prefix sum of the wave's 64 lanes
// (what the __shfl_up ladder gives); the ballot of the search is the count of the wave's lanes whose probe holds.
#include "stream_check_common.h"

namespace {

// the three passes of token_stream_table; returns table [n + 1] (exact size, caller frees)
int64_t* replay_table(const char* name, const Corpus& c) {
  const int64_t n = c.n, tiles = ddl::ts_tiles(n);
  int64_t* table = exact<int64_t>(n + 1);
  int64_t* sums = exact<int64_t>(tiles);
  std::vector<int> w_table(n + 1, 0), w_sums(tiles, 0);
  int64_t wave_tot[ddl::kTpWaves];
  std::vector<int64_t> len(ddl::kTpThreads), incl(ddl::kTpThreads);
  const auto scan_tile = [&](int64_t tile) {
    for (int t = 0; t < ddl::kTpThreads; ++t) {
      const int lane = t % ddl::kTpWave, wv = t / ddl::kTpWave;
      len[t] = ddl::ts_doc_len(c.offs_view(), c.n_corpus, c.order_view(), n, tile * ddl::kTpThreads + t);
      incl[t] = len[t] + (lane ? incl[t - 1] : 0);
      if (lane == ddl::kTpWave - 1) wave_tot[wv] = incl[t];
    }
  };
  for (int64_t tile = 0; tile < tiles; ++tile) {  // pass 1
    scan_tile(tile);
    sums[tile] = ddl::tp_before(wave_tot, ddl::kTpWaves, 0);
    ++w_sums[tile];
  }
  int64_t carry = 0;  // pass 2
  for (int64_t b = 0; b < tiles; b += ddl::kTpThreads) {
    std::vector<int64_t> v(ddl::kTpThreads), in(ddl::kTpThreads);
    for (int t = 0; t < ddl::kTpThreads; ++t) {
      const int lane = t % ddl::kTpWave, wv = t / ddl::kTpWave;
      v[t] = b + t < tiles ? sums[b + t] : 0;
      in[t] = v[t] + (lane ? in[t - 1] : 0);
      if (lane == ddl::kTpWave - 1) wave_tot[wv] = in[t];
    }
    int64_t next = 0;
    for (int t = 0; t < ddl::kTpThreads; ++t) {
      const int64_t before = ddl::tp_before(wave_tot, t / ddl::kTpWave, carry);
      if (b + t < tiles) {
        sums[b + t] = ddl::tp_exclusive(before, in[t], v[t]);
        ++w_sums[b + t];
      }
      if (t == ddl::kTpThreads - 1) next = before + in[t];
    }
    carry = next;
  }
  table[n] = carry;
  ++w_table[n];
  for (int64_t tile = 0; tile < tiles; ++tile) {  // pass 3
    scan_tile(tile);
    for (int t = 0; t < ddl::kTpThreads; ++t) {
      const int64_t i = tile * ddl::kTpThreads + t;
      if (i >= n) continue;
      table[i] = ddl::tp_exclusive(ddl::tp_before(wave_tot, t / ddl::kTpWave, sums[tile]), incl[t], len[t]);
      ++w_table[i];
    }
  }
  bool ok = true;
  int64_t tok = 0;
  for (int64_t i = 0; i < n; ++i) {
    ok = ok && w_table[i] == 1 && table[i] == tok;
    const int64_t q = c.order[i];
    if (q >= 0 && q < c.n_corpus && c.coffs[q + 1] > c.coffs[q]) tok += c.coffs[q + 1] - c.coffs[q];
  }
  ok = ok && w_table[n] == 1 && table[n] == tok;
  for (int64_t k = 0; k < tiles; ++k) ok = ok && w_sums[k] == 2;
  if (!ok) fail(name, "table mismatch");
  free(sums);
  return table;
}

void run_plan(const char* name, const Corpus& c, const int64_t* table, int64_t row_base, int64_t rows, int64_t S,
              int64_t max_segs) {
  ++g_cases;
  const int64_t n = c.n;
  int64_t* seg_offsets = exact<int64_t>(max_segs + 1);
  int64_t* seg_src = exact<int64_t>(max_segs);
  int64_t* row_start = exact<int64_t>(rows);
  int64_t* row_end = exact<int64_t>(rows);
  int64_t counts[4] = {-77, -77, -77, -77};
  std::vector<int> w_so(max_segs + 1, 0), w_ss(max_segs, 0);

  // ---- the kernel, replayed
  int64_t T0, T1;
  ddl::ts_window(row_base, rows, S, table[n], &T0, &T1);
  const int64_t n_tok = T1 - T0;
  int64_t carry_seg = 0, carry_max = 0;
  if (n_tok > 0) {
    const int64_t d0 = replay_search(name, table, n + 1, T0);
    const int64_t d1 = replay_search(name, table, n + 1, T1 - 1);
    if (!(table[d0] <= T0 && T0 < table[d0 + 1] && table[d1] <= T1 - 1 && T1 - 1 < table[d1 + 1]))
      fail(name, "search result");
    int64_t wave_seg[ddl::kTpWaves], wave_max[ddl::kTpWaves];
    std::vector<int64_t> a(ddl::kTpThreads), lo(ddl::kTpThreads), src0(ddl::kTpThreads), cc(ddl::kTpThreads),
        incl(ddl::kTpThreads);
    for (int64_t b = d0; b <= d1; b += ddl::kTpThreads) {
      for (int t = 0; t < ddl::kTpThreads; ++t) {
        const int lane = t % ddl::kTpWave, wv = t / ddl::kTpWave;
        int64_t mx;
        ddl::ts_plan_doc(c.offs_view(), c.n_corpus, c.table_view(), c.order_view(), n, b + t, d1, T0, T1, S, &a[t],
                         &lo[t], &src0[t], &cc[t], &mx);
        incl[t] = cc[t] + (lane ? incl[t - 1] : 0);
        if (lane == 0 || mx > wave_max[wv]) wave_max[wv] = mx;
        if (lane == ddl::kTpWave - 1) wave_seg[wv] = incl[t];
      }
      int64_t next = 0;
      for (int t = 0; t < ddl::kTpThreads; ++t) {
        const int64_t before = ddl::tp_before(wave_seg, t / ddl::kTpWave, carry_seg);
        const int64_t first = ddl::tp_exclusive(before, incl[t], cc[t]);
        const int64_t cnt = ddl::tp_seg_writes(first, cc[t], max_segs);
        if (cnt < 0 || cnt > cc[t]) fail(name, "segment write count out of range");
        for (int64_t j = 0; j < cnt; ++j) {
          if (first + j < 0 || first + j >= max_segs) {
            fail(name, "segment written past the capacity");
            continue;
          }
          const int64_t p = ddl::ts_piece_start(lo[t], j, S);
          seg_offsets[first + j] = p - T0;
          seg_src[first + j] = src0[t] + (p - a[t]);
          ++w_so[first + j], ++w_ss[first + j];
        }
        if (t == ddl::kTpThreads - 1) next = before + incl[t];
      }
      carry_seg = next;
      for (int k = 0; k < ddl::kTpWaves; ++k) carry_max = wave_max[k] > carry_max ? wave_max[k] : carry_max;
    }
  }
  for (int64_t r = 0; r < rows; ++r) {
    row_start[r] = ddl::ts_row_limit(r, S, n_tok);
    row_end[r] = ddl::ts_row_limit(r + 1, S, n_tok);
  }
  const int64_t n_seg = carry_seg;
  const bool fits = n_seg <= max_segs;
  if (fits) {
    seg_offsets[n_seg] = n_tok;
    ++w_so[n_seg];
  }
  counts[0] = fits ? ddl::ts_rows_used(n_tok, S) : -1;
  counts[1] = n_seg, counts[2] = n_tok, counts[3] = carry_max;

  // ---- the plain serial computation, token by token
  bool ok = true;
  int64_t seg = 0, mx = 0, run = 0, d = 0, prev_d = -1;
  for (int64_t g = T0; g < T1; ++g) {
    while (table[d + 1] <= g) ++d;  // the document holding g (empty ones are skipped)
    if (d != prev_d || g % S == 0) {  // a new piece
      if (seg < max_segs) {
        const int64_t q = c.order[d];
        ok = ok && w_so[seg] == 1 && w_ss[seg] == 1 && seg_offsets[seg] == g - T0 &&
             seg_src[seg] == c.coffs[q] + (g - table[d]);
      }
      ++seg;
      run = 0;
      prev_d = d;
    }
    ++run;
    mx = run > mx ? run : mx;
  }
  ok = ok && counts[1] == seg && counts[2] == T1 - T0 && counts[3] == mx;
  if (seg <= max_segs) {
    ok = ok && counts[0] == (n_tok + S - 1) / S && w_so[seg] == 1 && seg_offsets[seg] == n_tok;
    for (int64_t k = seg + 1; k <= max_segs; ++k) ok = ok && w_so[k] == 0;
    for (int64_t k = seg; k < max_segs; ++k) ok = ok && w_ss[k] == 0;
  } else {
    ok = ok && counts[0] == -1 && w_so[max_segs] == 0 && (max_segs == 0 || seg_offsets[0] == 0);
  }
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t s = r * S < n_tok ? r * S : n_tok, e = (r + 1) * S < n_tok ? (r + 1) * S : n_tok;
    ok = ok && row_start[r] == s && row_end[r] == e;
  }
  if (!ok) {
    printf("%s (n %lld, row_base %lld, rows %lld, S %lld, max_segs %lld): plan mismatch\n", name, (long long)n,
           (long long)row_base, (long long)rows, (long long)S, (long long)max_segs);
    ++g_failures;
  }
  for (void* p : {(void*)seg_offsets, (void*)seg_src, (void*)row_start, (void*)row_end}) free(p);
}

// lens: the corpus; order: the documents of the stream. A consistent order (in range) also runs the plan over
// windows at the start, in the middle, ending at T and reaching past it, at capacities that fit and that do not.
void run_case(const char* name, const std::vector<int64_t>& lens, const std::vector<int64_t>& order, bool plans) {
  ++g_cases;
  Corpus c = make_corpus(name, lens, order);
  const int64_t* table = c.table = replay_table(name, c);
  if (plans) {
    const int64_t T = table[c.n];
    for (int64_t S : {1, 4, 6, 37, 512}) {
      const int64_t total_rows = (T + S - 1) / S;
      for (int64_t rows : {1, 3, 7}) {
        for (int64_t row_base : {int64_t{0}, int64_t{1}, total_rows / 2, total_rows - rows, total_rows - 1,
                                 total_rows, total_rows + 5}) {
          if (row_base < 0) continue;
          const int64_t safe = rows * S + rows;  // >= the documents that touch the window + the row boundaries
          run_plan(name, c, table, row_base, rows, S, safe);
          run_plan(name, c, table, row_base, rows, S, 1);
          run_plan(name, c, table, row_base, rows, S, rows + 1);
        }
      }
    }
    run_plan(name, c, table, 0, T + 3, 1, T + 8);  // one token per row: as many pieces as tokens
    run_plan(name, c, table, 0, 2, T / 2 + 1, c.n + 4);  // the whole stream in two rows: every document walked
  }
  free_corpus(&c);
}

void run_all() {
  const std::vector<int64_t> lens13 = mod_lens(3001, 13), lens41 = mod_lens(3001, 41), ones = mod_lens(3001, 2, 1);
  for (int64_t n : {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 3001}) {  // wave and tile edges, the carries
    const std::vector<int64_t> order = stride_order(n, 7, 5, 3001);
    run_case("i % 13", lens13, order, true);
    run_case("i % 41", lens41, order, n <= 1025);
    run_case("1-2 tokens", ones, order, n >= 1024);  // > 1024 documents in one window: two plan tiles
  }
  run_case("all empty", std::vector<int64_t>(50, 0), mod_lens(1100, 50), true);
  std::vector<int64_t> edges = {0, 0, 5, 0, 0, 0, 7, 1, 0, 12, 0};  // runs of empty documents, also at both ends
  run_case("empty runs", edges, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, true);
  std::vector<int64_t> longs = {5000, 0, 4096, 4097, 1};  // documents over many rows: one lane, many pieces
  run_case("long documents", longs, {3, 1, 0, 4, 2}, true);
  // indices outside the corpus are never dereferenced (the table only: such an order has no consistent plan)
  run_case("out-of-range indices", lens41, {3, -1, 3001, 7, INT64_MIN, INT64_MAX, 3000, 0, -3001, 1 << 20}, false);
  std::vector<int64_t> bad_many;
  for (int64_t i = 0; i < 1500; ++i) bad_many.push_back(i % 3 == 0 ? 3001 + i : (i % 3 == 1 ? -i - 1 : i));
  run_case("out-of-range indices, two tiles", lens41, bad_many, false);
  run_case("empty corpus", {}, {0, 1, -1}, false);
  // more than 1024 tiles: the carry of the middle pass (1024 * 1024 + 5 documents)
  run_case("1024 * 1024 + 5 documents", mod_lens(977, 5), stride_order(1024 * 1024 + 5, 31, 7, 977), false);
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
  const int64_t* table = c.table = replay_table("far", c);
  if (table[c.n] <= (int64_t{1} << 43)) fail("far", "the stream is not far");
  for (int64_t S : {6, 37, 512}) {
    for (int64_t rows : {1, 3}) {
      std::vector<int64_t> bases = {((int64_t{1} << 32) + S - 1) / S, (int64_t{1} << 40) / S, (int64_t{1} << 43) / S - 1};
      for (int64_t i = 1; i <= c.n; ++i) bases.push_back(table[i] / S - 1);  // the rows across every document border
      for (int64_t row_base : bases) {
        run_plan("far", c, table, row_base, rows, S, rows * S + rows);
        run_plan("far", c, table, row_base, rows, S, 1);
      }
    }
  }
  free_corpus(&c);
}

}  // namespace

int main() {
  run_all();
  run_far();
  return finish("tokens stream check");
}
