// Host check of the batch descriptor kernel's index arithmetic (csrc/kernels/tokens_plan.h), built with
// -fsanitize=address,undefined by tests/test_resident_tokens_plan.py. It replays the kernel's loops
// (tokens_plan.hip) tile by tile, wave by wave, lane by lane on the host: the corpus offsets, the index and
// every output are heap buffers of exactly their size, so an offset read for an index outside the corpus, or a
// segment written past the capacity, is a heap overflow. Every read and write index is checked against the
// sizes as well, every output element must be written exactly once, and the result is compared with a plain
// serial loop. The wave scan is the serial prefix sum of the wave's 64 lanes (what the __shfl_up ladder gives).
#include "../tokens_plan.h"
#include "check_common.h"

namespace {

// lens: the corpus; idx: the selected sequences (any value: out-of-range ones are empty sequences)
void run_case(const char* name, const std::vector<int64_t>& lens, const std::vector<int64_t>& idx, int64_t S,
              int64_t max_segs) {
  ++g_cases;
  const int64_t n_corpus = static_cast<int64_t>(lens.size());
  const int64_t n = static_cast<int64_t>(idx.size());
  int64_t* coffs = exact<int64_t>(n_corpus + 1);
  coffs[0] = 0;
  for (int64_t i = 0; i < n_corpus; ++i) coffs[i + 1] = coffs[i] + lens[i];
  int64_t* index = exact<int64_t>(n);
  for (int64_t i = 0; i < n; ++i) index[i] = idx[i];
  int64_t* src_start = exact<int64_t>(n);
  int64_t* offsets = exact<int64_t>(n + 1);
  int64_t* seg_src = exact<int64_t>(max_segs);
  int64_t counts[4] = {-77, -77, -77, -77};
  std::vector<int> w_src(n, 0), w_off(n + 1, 0), w_seg(max_segs, 0);

  // ---- the kernel, replayed
  int64_t wave_tok[ddl::kTpWaves], wave_seg[ddl::kTpWaves], wave_max[ddl::kTpWaves];
  int64_t carry_tok = 0, carry_seg = 0, carry_max = 0;
  std::vector<int64_t> s0(ddl::kTpThreads), len(ddl::kTpThreads), c(ddl::kTpThreads), incl_tok(ddl::kTpThreads),
      incl_seg(ddl::kTpThreads);
  int64_t tiles = 0;
  for (int64_t b = 0; b < n; b += ddl::kTpThreads, ++tiles) {
    for (int t = 0; t < ddl::kTpThreads; ++t) {  // loads, the wave scans and the wave maximum
      const int64_t i = b + t;
      s0[t] = len[t] = 0;
      if (i < n) {
        const int64_t q = index[i];  // i < n: inside the index
        if (ddl::tp_index_ok(q, n_corpus)) {
          if (q < 0 || q + 1 > n_corpus) fail(name, "corpus offsets read out of range");
          s0[t] = coffs[q];
          len[t] = ddl::tp_len(s0[t], coffs[q + 1]);
        }
      }
      c[t] = ddl::tp_seg_count(len[t], S);
      const int lane = t % ddl::kTpWave, wv = t / ddl::kTpWave;
      incl_tok[t] = len[t] + (lane ? incl_tok[t - 1] : 0);
      incl_seg[t] = c[t] + (lane ? incl_seg[t - 1] : 0);
      const int64_t m = ddl::tp_seg_max(len[t], S);
      if (lane == 0 || m > wave_max[wv]) wave_max[wv] = m;
      if (lane == ddl::kTpWave - 1) {
        wave_tok[wv] = incl_tok[t];
        wave_seg[wv] = incl_seg[t];
      }
    }
    int64_t next_tok = 0, next_seg = 0;
    for (int t = 0; t < ddl::kTpThreads; ++t) {  // after the barrier
      const int64_t i = b + t;
      const int wv = t / ddl::kTpWave;
      const int64_t before_tok = ddl::tp_before(wave_tok, wv, carry_tok);
      const int64_t before_seg = ddl::tp_before(wave_seg, wv, carry_seg);
      if (i < n) {
        src_start[i] = s0[t];
        offsets[i] = ddl::tp_exclusive(before_tok, incl_tok[t], len[t]);
        ++w_src[i], ++w_off[i];
      }
      const int64_t first = ddl::tp_exclusive(before_seg, incl_seg[t], c[t]);
      const int64_t cnt = ddl::tp_seg_writes(first, c[t], max_segs);
      if (cnt < 0 || cnt > c[t]) fail(name, "segment write count out of range");
      for (int64_t j = 0; j < cnt; ++j) {
        if (first + j < 0 || first + j >= max_segs) {
          fail(name, "segment written past the capacity");
          continue;
        }
        seg_src[first + j] = ddl::tp_seg_src(s0[t], j, S);
        ++w_seg[first + j];
      }
      if (t == ddl::kTpThreads - 1) {
        next_tok = before_tok + incl_tok[t];
        next_seg = before_seg + incl_seg[t];
      }
    }
    carry_tok = next_tok, carry_seg = next_seg;
    for (int k = 0; k < ddl::kTpWaves; ++k) carry_max = wave_max[k] > carry_max ? wave_max[k] : carry_max;
  }
  if (tiles != ddl::tp_tiles(n)) fail(name, "tile count");
  offsets[n] = carry_tok;
  ++w_off[n];
  counts[2] = carry_tok;
  counts[3] = carry_max;

  // ---- the plain serial computation
  bool ok = counts[0] == -77 && counts[1] == -77;  // the plan kernel's slots are left alone
  int64_t tok = 0, seg = 0, mx = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t q = idx[i];
    const bool in = q >= 0 && q < n_corpus;
    const int64_t start = in ? coffs[q] : 0, l = in ? lens[q] : 0;
    ok = ok && w_src[i] == 1 && w_off[i] == 1 && src_start[i] == start && offsets[i] == tok;
    for (int64_t j = 0; j * S < l; ++j, ++seg)
      if (seg < max_segs) ok = ok && w_seg[seg] == 1 && seg_src[seg] == start + j * S;
    tok += l;
    mx = (l < S ? l : S) > mx ? (l < S ? l : S) : mx;
  }
  for (int64_t k = seg; k < max_segs; ++k) ok = ok && w_seg[k] == 0;  // nothing past the batch's segments
  ok = ok && w_off[n] == 1 && offsets[n] == tok && counts[2] == tok && counts[3] == mx && carry_seg == seg;
  if (!ok) {
    printf("%s (n %lld, S %lld, max_segs %lld): mismatch\n", name, (long long)n, (long long)S, (long long)max_segs);
    ++g_failures;
  }
  for (void* p : {(void*)coffs, (void*)index, (void*)src_start, (void*)offsets, (void*)seg_src}) free(p);
}

void run_all() {
  // the corpus of the GPU tests: lengths i % 13 (every 13th sequence is empty)
  const std::vector<int64_t> lens13 = mod_lens(3001, 13);
  const std::vector<int64_t> lens41 = mod_lens(3001, 41);  // up to 40 tokens: 7 segments at S = 6
  for (int64_t n : {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049}) {  // wave and tile edges, the carry across tiles
    const std::vector<int64_t> idx = stride_order(n, 7, 5, 3001);
    run_case("i % 13", lens13, idx, 37, 2 * n + 1);
    run_case("i % 13, short rows", lens13, idx, 6, 2 * n + 1);
    run_case("i % 41, many segments", lens41, idx, 6, 7 * n + 1);
    run_case("i % 41, exact capacity", lens41, idx, 4096, n);
    run_case("i % 41, capacity exceeded", lens41, idx, 6, n);      // segments > max_segs: clipped
    run_case("i % 41, no capacity", lens41, idx, 6, 0);
  }
  run_case("all empty", std::vector<int64_t>(50, 0), mod_lens(1100, 50), 16, 8);
  // indices outside the corpus are never dereferenced
  std::vector<int64_t> bad = {3, -1, 3001, 7, INT64_MIN, INT64_MAX, 3000, 0, -3001, 1 << 20};
  run_case("out-of-range indices", lens41, bad, 6, 64);
  std::vector<int64_t> bad_many;
  for (int64_t i = 0; i < 1500; ++i) bad_many.push_back(i % 3 == 0 ? 3001 + i : (i % 3 == 1 ? -i - 1 : i));
  run_case("out-of-range indices, two tiles", lens41, bad_many, 6, 4000);
  run_case("empty corpus", {}, {0, 1, -1}, 6, 4);
  // long sequences: one lane writes many segments, and the longest segment is S
  std::vector<int64_t> longs = {5000, 0, 4096, 4097, 1};
  run_case("long sequences", longs, {0, 1, 2, 3, 4, 0}, 4096, 16);
  run_case("long sequences, S = 1", longs, {3, 4}, 1, 5000);
}

// Far corpus: eight documents of 2^40 tokens among short and empty ones, one of 2^32 + 3, so that the corpus
// offsets, the table and every seg_src pass 2^32 and 2^40 and reach 2^43. Nothing of that size is materialised.
std::vector<int64_t> far_lens() {
  const int64_t big = int64_t{1} << 40;
  return {5, big, 0, 7, big, big, 1, (int64_t{1} << 32) + 3, big, 0, 0, big, 4097, big, big, 3, big, 11};
}

// The batch descriptor over the far corpus: src_start and seg_src past 2^43, offsets (the batch's running token
// count) past 2^41. The rows are long enough that a 2^40-token sequence makes 512 or 3 segments, not 2^37.
void run_far() {
  const std::vector<int64_t> lens = far_lens();
  const std::vector<int64_t> idx = {16, 3, 1, 9, 7, 0, 13, -1, 2, 4, 17, 18, 16, 8};
  run_case("far, S = 2^31", lens, idx, int64_t{1} << 31, 4096);
  run_case("far, S = 2^31, capacity exceeded", lens, idx, int64_t{1} << 31, 1000);
  run_case("far, S = 2^39 + 1", lens, idx, (int64_t{1} << 39) + 1, 64);
  run_case("far, S = 2^31 - 1", lens, idx, (int64_t{1} << 31) - 1, 4096);
}

}  // namespace

int main() {
  run_all();
  run_far();
  return finish("tokens plan check");
}
