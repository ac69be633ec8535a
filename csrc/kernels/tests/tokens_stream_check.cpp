// Host check of the token stream kernels' index arithmetic (csrc/kernels/tokens_stream.h), built with
// -fsanitize=address,undefined by tests/test_token_stream.py. It replays the kernels' loops (tokens_stream.hip)
// tile by tile, wave by wave, lane by lane on the host: the corpus offsets, the order, the table, the tile sums
// and every plan array are heap buffers of exactly their size, so an offset read for an index outside the corpus,
// a probe past the table or a segment written past the capacity is a heap overflow. Every write index is checked
// against the sizes as well, every output element must be written exactly once, and the results are compared
// with plain serial loops. The wave scan is the serial prefix sum of the wave's 64 lanes (what the __shfl_up
// ladder gives); the ballot of the search is the count of the wave's lanes whose probe holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../tokens_stream.h"

namespace {

int g_failures = 0;

void fail(const char* name, const char* what) {
  printf("%s: %s\n", name, what);
  ++g_failures;
}

template <typename T>
T* exact(size_t n) {  // exactly n elements (n = 0: a one-byte block nothing may touch as a T)
  return static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
}

struct Corpus {
  int64_t n_corpus;
  int64_t* coffs;  // [n_corpus + 1]
  int64_t n;
  int64_t* order;  // [n]: any value (out-of-range ones are empty documents)
};

int64_t doc_len(const Corpus& c, int64_t i, const char* name) {  // ts_doc_len
  if (i >= c.n) return 0;
  const int64_t q = c.order[i];
  if (!ddl::tp_index_ok(q, c.n_corpus)) return 0;
  if (q < 0 || q + 1 > c.n_corpus) fail(name, "corpus offsets read out of range");
  return ddl::tp_len(c.coffs[q], c.coffs[q + 1]);
}

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
      len[t] = doc_len(c, tile * ddl::kTpThreads + t, name);
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

// ts_wave_last_le: the 64 lanes of one wave
int64_t replay_search(const char* name, const int64_t* table, int64_t n1, int64_t v) {
  int64_t lo = 0, hi = n1;
  int steps = 0;
  while (hi - lo > 1) {
    const int64_t stride = ddl::ts_search_stride(lo, hi);
    int k = 0;
    for (int lane = 0; lane < ddl::kTpWave; ++lane) {
      const int64_t p = ddl::ts_search_probe(lo, stride, lane);
      if (p < hi) {
        if (p < 0 || p >= n1) fail(name, "search probe outside the table");
        if (table[p] <= v) ++k;
      }
    }
    if (k < 1) k = 1;
    ddl::ts_search_narrow(&lo, &hi, stride, k);
    if (++steps > 64) {
      fail(name, "search does not terminate");
      break;
    }
  }
  return lo;
}

void run_plan(const char* name, const Corpus& c, const int64_t* table, int64_t row_base, int64_t rows, int64_t S,
              int64_t max_segs) {
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
        const int64_t d = b + t;
        int64_t hi = 0, mx = 0;
        a[t] = lo[t] = src0[t] = cc[t] = 0;
        if (d <= d1 && d < n) {
          const int64_t q = c.order[d];
          a[t] = table[d];
          if (ddl::tp_index_ok(q, c.n_corpus) && ddl::ts_clip(a[t], table[d + 1], T0, T1, &lo[t], &hi)) {
            if (q < 0 || q >= c.n_corpus) fail(name, "corpus offsets read out of range");
            src0[t] = c.coffs[q];
            cc[t] = ddl::ts_pieces(lo[t], hi, S);
            mx = ddl::ts_piece_max(lo[t], hi, S);
          }
        }
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
  Corpus c;
  c.n_corpus = static_cast<int64_t>(lens.size());
  c.n = static_cast<int64_t>(order.size());
  c.coffs = exact<int64_t>(c.n_corpus + 1);
  c.coffs[0] = 0;
  for (int64_t i = 0; i < c.n_corpus; ++i) c.coffs[i + 1] = c.coffs[i] + lens[i];
  c.order = exact<int64_t>(c.n);
  for (int64_t i = 0; i < c.n; ++i) c.order[i] = order[i];
  int64_t* table = replay_table(name, c);
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
  free(table);
  free(c.coffs);
  free(c.order);
}

void run_all() {
  std::vector<int64_t> lens13, lens41, ones;
  for (int64_t i = 0; i < 3001; ++i) {
    lens13.push_back(i % 13);  // every 13th document is empty
    lens41.push_back(i % 41);
    ones.push_back(1 + i % 2);
  }
  for (int64_t n : {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 3001}) {  // wave and tile edges, the carries
    std::vector<int64_t> order;
    for (int64_t i = 0; i < n; ++i) order.push_back((i * 7 + 5) % 3001);
    run_case("i % 13", lens13, order, true);
    run_case("i % 41", lens41, order, n <= 1025);
    run_case("1-2 tokens", ones, order, n >= 1024);  // > 1024 documents in one window: two plan tiles
  }
  std::vector<int64_t> empty(50, 0), all;
  for (int64_t i = 0; i < 1100; ++i) all.push_back(i % 50);
  run_case("all empty", empty, all, true);
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
  std::vector<int64_t> big_lens(977), big_order;
  for (int64_t i = 0; i < 977; ++i) big_lens[i] = i % 5;
  for (int64_t i = 0; i < 1024 * 1024 + 5; ++i) big_order.push_back((i * 31 + 7) % 977);
  run_case("1024 * 1024 + 5 documents", big_lens, big_order, false);
}

}  // namespace

int main() {
  run_all();
  if (g_failures) {
    printf("tokens stream check: %d failures\n", g_failures);
    return 1;
  }
  printf("tokens stream check ok\n");
  return 0;
}
