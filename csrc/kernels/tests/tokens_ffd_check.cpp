// Host check of the first-fit-decreasing order kernel's index arithmetic (csrc/kernels/tokens_ffd.h), built with
// -fsanitize=address,undefined by tests/test_token_ffd.py. It replays the kernel's steps (tokens_ffd.hip) lane by
// lane on the host -- the item words, the bitonic sort's compare-exchanges, the placing wave's ballots over the
// groups' maxima and over a group's 64 bins, the scan of the bins' sizes and every sequence's place -- over heap
// buffers of exactly their size, so a read or a write outside them is a heap overflow; every index is checked
// against the sizes as well, and every output element must be written exactly once. The result is compared with a
// straight transcription of the definition (ddl_amd.models.tokens.ffd_order_py / in_order_rows_py /
// ffd_if_it_wins). A wave reduction is the plain maximum over the wave's 64 lanes.
#include "../tokens_ffd.h"
#include "../tokens_plan.h"
#include "check_common.h"

namespace {

constexpr int W = ddl::kFfdWave;

int first_bit(const bool* m) {  // __ffsll(__ballot(m)) - 1
  for (int l = 0; l < W; ++l)
    if (m[l]) return l;
  return -1;
}

// ---- the definition
void definition(const std::vector<int64_t>& lens, int64_t S, std::vector<int64_t>* order, int64_t* ffd_rows,
                int64_t* in_order) {
  const int64_t n = static_cast<int64_t>(lens.size());
  std::vector<int64_t> rem(n), items;
  int64_t full = 0;
  for (int64_t i = 0; i < n; ++i) {
    rem[i] = lens[i] > S ? lens[i] % S : lens[i];
    full += lens[i] > S ? lens[i] / S : 0;
    if (rem[i] > 0) items.push_back(i);
  }
  for (size_t a = 1; a < items.size(); ++a) {  // a stable insertion sort by descending size
    const int64_t x = items[a];
    size_t b = a;
    for (; b > 0 && rem[items[b - 1]] < rem[x]; --b) items[b] = items[b - 1];
    items[b] = x;
  }
  std::vector<int64_t> left;
  std::vector<bool> has_long;
  std::vector<std::vector<int64_t>> bins;
  for (int64_t i : items) {
    const bool lng = lens[i] > S;
    size_t b = 0;
    for (; b < bins.size(); ++b)
      if (left[b] >= rem[i] && !(lng && has_long[b])) break;
    if (b == bins.size()) {
      bins.emplace_back();
      left.push_back(S);
      has_long.push_back(false);
    }
    bins[b].push_back(i);
    left[b] -= rem[i];
    if (lng) has_long[b] = true;
  }
  order->clear();
  for (const auto& members : bins) {
    for (int64_t i : members)
      if (lens[i] > S) order->push_back(i);
    for (int64_t i : members)
      if (lens[i] <= S) order->push_back(i);
  }
  for (int64_t i = 0; i < n; ++i)
    if (rem[i] == 0) order->push_back(i);
  *ffd_rows = static_cast<int64_t>(bins.size()) + full;
  int64_t rows = 0, cur = S;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t l = lens[i]; l > 0;) {
      const int64_t seg = l < S ? l : S;
      if (seg > S - cur) ++rows, cur = 0;
      cur += seg;
      l -= seg;
    }
  *in_order = rows;
}

// lens: the corpus; idx: the selected sequences (any value: out-of-range ones are empty sequences)
void run_case(const char* name, const std::vector<int64_t>& lens, const std::vector<int64_t>& idx, int64_t S,
              int want_used = -1) {
  ++g_cases;
  const int64_t n_corpus = static_cast<int64_t>(lens.size());
  const int64_t n = static_cast<int64_t>(idx.size());
  if (n > ddl::kFfdMaxSeqs) return fail(name, "case larger than the kernel takes");
  int64_t* coffs = exact<int64_t>(n_corpus + 1);
  coffs[0] = 0;
  for (int64_t i = 0; i < n_corpus; ++i) coffs[i + 1] = coffs[i] + lens[i];
  int64_t* index = exact<int64_t>(n);
  for (int64_t i = 0; i < n; ++i) index[i] = idx[i];
  int64_t* index_out = exact<int64_t>(n);
  int64_t counts[3] = {-77, -77, -77};
  std::vector<int> w_out(n, 0);

  std::vector<int64_t> sel_lens(n);
  for (int64_t i = 0; i < n; ++i) sel_lens[i] = idx[i] >= 0 && idx[i] < n_corpus ? lens[idx[i]] : 0;

  // ---- the kernel, replayed; the LDS arrays at the sizes the kernel declares
  const int64_t cap = ddl::kFfdMaxSeqs;
  uint64_t* item = exact<uint64_t>(cap);
  uint64_t* skey = exact<uint64_t>(cap);
  uint64_t* bins = exact<uint64_t>(cap);
  uint16_t* spos = exact<uint16_t>(cap);
  uint16_t* n_short = exact<uint16_t>(cap);
  uint16_t* bin_of = exact<uint16_t>(cap);
  uint16_t* rank_of = exact<uint16_t>(cap);
  if (n == 0) {
    counts[0] = counts[1] = counts[2] = 0;
  } else {
    const int64_t P = ddl::ffd_sort_size(n);
    if (P > cap || P < n || (P & (P - 1))) fail(name, "sort size");
    int64_t full = 0;
    for (int64_t i = 0; i < P; ++i) {  // 1. item words (lane i % 1024)
      uint64_t w = 0;
      if (i < n) {
        const int64_t q = index[i];
        int64_t len = 0;
        if (ddl::tp_index_ok(q, n_corpus)) {
          if (q < 0 || q + 1 > n_corpus) fail(name, "corpus offsets read out of range");
          len = ddl::tp_len(coffs[q], coffs[q + 1]);
        }
        w = ddl::ffd_item(len, S);
        full += ddl::ffd_full_rows(len, S);
        item[i] = w;
      }
      skey[i] = w;
      spos[i] = static_cast<uint16_t>(i);
    }
    for (int64_t k = 2; k <= P; k <<= 1)  // 2. the bitonic sort
      for (int64_t j = k >> 1; j > 0; j >>= 1) {
        std::vector<int> touched(P, 0);
        for (int64_t p = 0; p < (P >> 1); ++p) {
          const int64_t lo = ddl::ffd_pair_lo(p, j), hi = lo + j;
          if (lo < 0 || hi >= P) {
            fail(name, "compare-exchange outside the sort");
            continue;
          }
          ++touched[lo], ++touched[hi];
          if (ddl::ffd_before(skey[hi], spos[hi], skey[lo], spos[lo]) == ddl::ffd_pair_forward(lo, k)) {
            const uint64_t w = skey[lo];
            skey[lo] = skey[hi], skey[hi] = w;
            const uint16_t s = spos[lo];
            spos[lo] = spos[hi], spos[hi] = s;
          }
        }
        for (int64_t i = 0; i < P; ++i)
          if (touched[i] != 1) fail(name, "a sort step does not touch every element once");
      }
    for (int64_t m = 1; m < P; ++m)
      if (!ddl::ffd_before(skey[m - 1], spos[m - 1], skey[m], spos[m])) fail(name, "not sorted");
    // 3. wave 0: the placement (lane g keeps group g's maxima)
    int64_t max_short[W], max_long[W];
    for (int l = 0; l < W; ++l) max_short[l] = max_long[l] = -1;
    int64_t n_bins = 0, m = 0;
    for (; m < n; ++m) {
      const uint64_t it = skey[m];
      const int64_t s = ddl::ffd_item_size(it);
      if (s == 0) break;
      const bool lng = ddl::ffd_item_long(it);
      bool ballot[W];
      for (int l = 0; l < W; ++l) ballot[l] = (lng ? max_long[l] : max_short[l]) >= s;
      const int g = first_bit(ballot);
      uint64_t w[W];
      int slot = -1;
      if (g >= 0) {
        for (int l = 0; l < W; ++l) {
          const int64_t b = ddl::ffd_bin(g, l);
          if (b < 0 || b >= cap) fail(name, "bin read out of range");
          w[l] = b < n_bins ? bins[b] : 0;
          ballot[l] = b < n_bins && ddl::ffd_room(w[l], lng) >= s;
        }
        slot = first_bit(ballot);
        if (slot < 0) fail(name, "a group's maximum promised room that no bin has");
      }
      if (slot >= 0) {
        const int64_t b = ddl::ffd_bin(g, slot);
        const uint64_t old = w[slot];
        w[slot] = ddl::ffd_bin_take(old, it);
        bins[b] = w[slot];
        rank_of[m] = n_short[b];
        if (!lng) n_short[b] = n_short[b] + 1;
        bin_of[m] = static_cast<uint16_t>(b);
        int64_t ms = -1, ml = -1;
        for (int l = 0; l < W; ++l)
          if (ddl::ffd_bin(g, l) < n_bins) {
            ms = ddl::ffd_room_short(w[l]) > ms ? ddl::ffd_room_short(w[l]) : ms;
            ml = ddl::ffd_room_long(w[l]) > ml ? ddl::ffd_room_long(w[l]) : ml;
          }
        if (ddl::ffd_needs_refresh(old, max_short[g], max_long[g])) {
          max_short[g] = ms, max_long[g] = ml;
        } else if (max_short[g] != ms || max_long[g] != ml) {
          fail(name, "a skipped refresh left a stale maximum");
        }
      } else {
        const int64_t b = n_bins++;
        if (b >= cap) {
          fail(name, "more bins than the tree holds");
          break;
        }
        const uint64_t nw = ddl::ffd_bin_open(S, it);
        bins[b] = nw;
        rank_of[m] = 0;
        n_short[b] = lng ? 0 : 1;
        bin_of[m] = static_cast<uint16_t>(b);
        const int gg = ddl::ffd_group(b);
        if (gg < 0 || gg >= W || ddl::ffd_bin(gg, ddl::ffd_slot(b)) != b) fail(name, "tree addressing");
        max_short[gg] = ddl::ffd_room_short(nw) > max_short[gg] ? ddl::ffd_room_short(nw) : max_short[gg];
        max_long[gg] = ddl::ffd_room_long(nw) > max_long[gg] ? ddl::ffd_room_long(nw) : max_long[gg];
      }
    }
    const int64_t n_items = m;
    int64_t rows = 0, cur = S;  // lane 0 of wave 1: the next-fit
    for (int64_t i = 0; i < n; ++i) ddl::ffd_next_fit(item[i], S, &rows, &cur);
    // 4. the bins' starts and the places
    counts[0] = n_bins + full;
    counts[1] = rows + full;
    counts[2] = counts[0] < counts[1] ? 1 : 0;
    if (!counts[2]) {
      for (int64_t i = 0; i < n; ++i) index_out[i] = index[i], ++w_out[i];
    } else {
      int64_t start = 0;
      for (int64_t b = 0; b < cap; ++b) {  // the scan, four bins per lane
        const int64_t size = b < n_bins ? ddl::ffd_bin_size(n_short[b], bins[b]) : 0;
        item[b] = static_cast<uint64_t>(start);
        start += size;
      }
      for (int64_t k = 0; k < n; ++k) {
        int64_t at = k;
        if (k < n_items) {
          const int64_t b = bin_of[k];
          if (b >= n_bins) fail(name, "bin of an item out of range");
          at = ddl::ffd_position(static_cast<int64_t>(item[b]), ddl::ffd_item_long(skey[k]), rank_of[k], bins[b]);
        }
        if (at < 0 || at >= n || spos[k] >= n) {
          fail(name, "index written or read out of range");
          continue;
        }
        index_out[at] = index[spos[k]];
        ++w_out[at];
      }
    }
  }

  // ---- against the definition
  std::vector<int64_t> order;
  int64_t ffd_rows = 0, in_order = 0;
  definition(sel_lens, S, &order, &ffd_rows, &in_order);
  const int used = ffd_rows < in_order ? 1 : 0;
  bool ok = counts[0] == ffd_rows && counts[1] == in_order && counts[2] == used;
  for (int64_t i = 0; i < n; ++i) ok = ok && w_out[i] == 1 && index_out[i] == idx[used ? order[i] : i];
  if (want_used >= 0 && used != want_used) fail(name, "the case does not exercise the branch it is meant for");
  if (!ok) {
    printf("%s (n %lld, S %lld): mismatch (rows %lld / %lld, want %lld / %lld)\n", name, (long long)n, (long long)S,
           (long long)counts[0], (long long)counts[1], (long long)ffd_rows, (long long)in_order);
    ++g_failures;
  }
  for (void* p : {(void*)coffs, (void*)index, (void*)index_out, (void*)item, (void*)skey, (void*)bins, (void*)spos,
                  (void*)n_short, (void*)bin_of, (void*)rank_of})
    free(p);
}

std::vector<int64_t> iota(int64_t n) { return stride_order(n, 1, 0, n > 0 ? n : 1); }

void run_all() {
  Lcg rng{12345};
  for (int64_t S : {8, 37, 4096}) {
    for (int64_t n : {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4096}) {
      run_case("all equal", std::vector<int64_t>(n, S / 3 + 1), iota(n), S);
      run_case("all equal, S", std::vector<int64_t>(n, S), iota(n), S);
      std::vector<int64_t> rnd(n), mixed(n), pairs(n), tiny(n);
      const int64_t special[] = {0, S, 2 * S, S + 1, 3 * S - 1};
      for (int64_t i = 0; i < n; ++i) {
        rnd[i] = 1 + rng.next() % (2 * S);
        mixed[i] = i % 3 == 0 ? special[(i / 3) % 5] : 1 + rng.next() % S;
        pairs[i] = S / 2;
        tiny[i] = i % 4 == 0 ? S * (1 + i % 3) + 1 + i % 2 : 1 + rng.next() % (S / 2);
      }
      run_case("random in [1, 2S]", rnd, iota(n), S);
      run_case("0, S, 2S, S + 1, 3S - 1 mixed in", mixed, iota(n), S);
      if (S % 2 == 0) run_case("in-order pairs", pairs, iota(n), S, 0);
      run_case("long sequences with tiny remainders", tiny, iota(n), S);
      // a corpus read through an index with entries outside it
      std::vector<int64_t> idx = stride_order(n, 7, 5, n > 0 ? n : 1);
      for (int64_t i = 0; i < n; i += 17) idx[i] = i % 2 ? -1 - i : n + i;
      run_case("out-of-range indices", rnd, idx, S);
    }
    run_case("200 bins", std::vector<int64_t>(200, S / 2 + 1), iota(200), S);
    run_case("the full tree", std::vector<int64_t>(4096, S / 2 + 1), iota(4096), S);
    std::vector<int64_t> win = {S - 1, 2, S - 2, 1, 1, S - 1, 2, S - 2};  // FFD wins: used = 1
    run_case("ffd wins", win, iota(8), S, 1);
  }
  run_case("empty corpus", {}, {0, 1, -1}, 6);
  run_case("S = 1", {5, 0, 1, 1, 7}, {0, 1, 2, 3, 4}, 1);
  // far: lengths and row sizes past 2^32 and 2^40 (nothing of that size is materialised)
  const int64_t big = int64_t{1} << 40;
  const std::vector<int64_t> far = {5, big, 0, 7, big + 3, big, 1, (int64_t{1} << 32) + 3, 2 * big, 0, 4097, big - 1};
  const std::vector<int64_t> far_idx = {11, 3, 1, 9, 7, 0, 10, -1, 2, 4, 12, 8, 5, 6};
  for (int64_t S : {int64_t{4096}, int64_t{1} << 31, (int64_t{1} << 39) + 1, big, INT64_MAX})
    run_case("far", far, far_idx, S);
}

}  // namespace

int main() {
  run_all();
  return finish("tokens ffd check");
}
