// Host check of the fill-in-the-middle kernel (tokens_fim.hip): the kernel's per-lane routine tf_lane4 of tokens_fim.h
// replayed for every lane of every workgroup of the kernel's grid, over exact-size buffers whose views name an index
// outside them before the load, against batches rearranged independently here: every segment's layout written out
// piece by piece (sentinel, prefix, sentinel, suffix, ...) into a vector, and the labels read off the result.
// Stand-alone: no HIP. Built with -fsanitize=address,undefined (tests/host_check.py).
#include "../tokens_fim.h"
#include "check_common.h"

namespace {

template <typename T>
struct Checked {  // n elements of an exact-size buffer; an index outside is named before the load
  const T* p;
  int64_t n;
  const char* name;
  const char* what;
  T operator()(int64_t i) const {
    if (i < 0 || i >= n) {
      fail(name, what);
      return T{};
    }
    return p[i];
  }
};

struct Batch {
  int64_t R, S, cap;
  std::vector<int32_t> ids, cu;
  std::vector<int64_t> seg, pos, keys;
};

// rows filled with segments of the given lengths in turn (a segment never crosses a row: it is cut there), the
// last `pad_tail` columns of every row padding; about half the segments end in `eod`
Batch make_batch(int64_t R, int64_t S, const std::vector<int64_t>& lens, int64_t pad_tail, int32_t eod, Lcg* rng) {
  Batch b;
  b.R = R, b.S = S;
  b.ids.assign(R * S, 0), b.seg.assign(R * S, -1), b.pos.assign(R * S, 0);
  b.cu.push_back(0);
  size_t li = 0;
  for (int64_t r = 0; r < R; ++r) {
    int64_t c = 0;
    const int64_t width = S - (pad_tail < S ? pad_tail : 0);
    while (c < width) {
      int64_t L = lens[li++ % lens.size()];
      if (L < 1) continue;
      if (L > width - c) L = width - c;
      const int64_t s = static_cast<int64_t>(b.cu.size()) - 1;
      for (int64_t j = 0; j < L; ++j) {
        b.ids[r * S + c + j] = 1 + static_cast<int32_t>(rng->next() % 40000);
        b.seg[r * S + c + j] = s;
        b.pos[r * S + c + j] = j;
      }
      if (rng->next() % 2) b.ids[r * S + c + L - 1] = eod;
      if (L > 2 && rng->next() % 4 == 0) b.ids[r * S + c + L / 2] = eod;  // an EOD mid-way changes nothing
      b.cu.push_back(b.cu.back() + static_cast<int32_t>(L));
      b.keys.push_back((rng->next() << 31) ^ rng->next());
      c += L;
    }
  }
  b.cap = static_cast<int64_t>(b.keys.size());
  return b;
}

// the definition, written out: one segment t with its draws
std::vector<int32_t> written_segment(const ddl::FimParams& fp, const std::vector<int32_t>& t, uint64_t key, int* kind) {
  uint64_t u[4];
  for (uint64_t c = 0; c < 4; ++c) u[c] = ddl::tf_mix64(fp.ekey ^ ddl::tf_mix64(4 * key + c));
  const int64_t L = static_cast<int64_t>(t.size());
  const int64_t tail = fp.has_eod && t[L - 1] == fp.eod_id ? 1 : 0;
  const int64_t M = L - tail, K = M - 3;
  *kind = 0;
  if (M < fp.min_len || (u[0] >> 40) >= fp.rate_q) return t;
  const int64_t x = static_cast<int64_t>(((u[2] >> 32) * static_cast<uint64_t>(K + 1)) >> 32);
  const int64_t y = static_cast<int64_t>(((u[3] >> 32) * static_cast<uint64_t>(K + 1)) >> 32);
  const int64_t a = x < y ? x : y, b = x < y ? y : x;
  const std::vector<int32_t> pre(t.begin(), t.begin() + a), mid(t.begin() + a, t.begin() + b),
      suf(t.begin() + b, t.begin() + K);
  std::vector<int32_t> out;
  out.push_back(fp.prefix_id);
  if ((u[1] >> 40) < fp.spm_q) {
    *kind = 2;
    out.push_back(fp.suffix_id);
    out.insert(out.end(), suf.begin(), suf.end());
    out.push_back(fp.middle_id);
    out.insert(out.end(), pre.begin(), pre.end());
    out.insert(out.end(), mid.begin(), mid.end());
  } else {
    *kind = 1;
    out.insert(out.end(), pre.begin(), pre.end());
    out.push_back(fp.suffix_id);
    out.insert(out.end(), suf.begin(), suf.end());
    out.push_back(fp.middle_id);
    out.insert(out.end(), mid.begin(), mid.end());
  }
  if (tail) out.push_back(t[L - 1]);
  return out;
}

int64_t g_kinds[3] = {0, 0, 0};

// the kernel over batch b: ti_chunks(S) workgroups per row of kTiThreads lanes, lane = 4 positions. sound: the batch
// is one make_batch built, so the outputs are compared with its segments' layouts; otherwise (a corrupt batch) with the
// soundness rule written out position by position.
void replay(const char* name, const Batch& b, const ddl::FimParams& fp, bool live, bool sound) {
  ++g_cases;
  const int64_t R = b.R, S = b.S, n = R * S;
  int32_t* ids = exact<int32_t>(n);
  int32_t* cu = exact<int32_t>(b.cu.size());
  int64_t* keys = exact<int64_t>(b.keys.size());
  for (int64_t i = 0; i < n; ++i) ids[i] = b.ids[i];
  for (size_t i = 0; i < b.cu.size(); ++i) cu[i] = b.cu[i];
  for (size_t i = 0; i < b.keys.size(); ++i) keys[i] = b.keys[i];
  std::vector<int32_t> out(n, -7);
  std::vector<int64_t> lab(n, -7);
  std::vector<int> writes(n, 0);
  const Checked<int32_t> cu_v{cu, static_cast<int64_t>(b.cu.size()), name, "cu_seqlens read out of range"};
  const Checked<int64_t> key_v{keys, static_cast<int64_t>(b.keys.size()), name, "seg_keys read out of range"};
  const int32_t chunks = static_cast<int32_t>(ddl::ti_chunks(S));
  const int64_t grid = ddl::ti_grid(R, 0, S, false);
  if (grid != R * chunks) fail(name, "grid is not one workgroup per (row, chunk)");
  for (int64_t bx = 0; bx < grid; ++bx) {
    for (int t = 0; t < ddl::kTiThreads; ++t) {
      int64_t row, p0;
      ddl::ti_lane_origin(static_cast<uint32_t>(bx), chunks, t, &row, &p0);
      if (row >= R || p0 >= S) continue;
      int64_t seg[4] = {-1, -1, -1, -1}, pos[4] = {0, 0, 0, 0};
      int32_t own[4] = {0, 0, 0, 0}, o4[4];
      int64_t l4[4];
      for (int k = 0; k < 4 && p0 + k < S; ++k) {
        seg[k] = b.seg[row * S + p0 + k];
        pos[k] = b.pos[row * S + p0 + k];
        own[k] = ids[row * S + p0 + k];
      }
      const Checked<int32_t> row_v{ids + row * S, S, name, "token read outside the row"};
      ddl::tf_lane4(fp, S, b.cap, live, p0, seg, pos, own, cu_v, key_v, row_v, true, -100, o4, l4);
      for (int k = 0; k < 4 && p0 + k < S; ++k) {
        out[row * S + p0 + k] = o4[k];
        lab[row * S + p0 + k] = l4[k];
        ++writes[row * S + p0 + k];
      }
    }
  }
  for (int64_t i = 0; i < n; ++i)
    if (writes[i] != 1) {
      fail(name, "a position is not written exactly once");
      break;
    }
  if (sound) {
    std::vector<int32_t> want(b.ids);
    std::vector<int64_t> want_lab(n, -100);
    std::vector<int64_t> first(b.cap, -1);
    for (int64_t i = n - 1; i >= 0; --i)
      if (b.seg[i] >= 0) first[b.seg[i]] = i;
    for (int64_t s = 0; s < b.cap; ++s) {
      const int64_t at = first[s];
      const int64_t L = b.cu[s + 1] - b.cu[s];
      const std::vector<int32_t> t(b.ids.begin() + at, b.ids.begin() + at + L);
      int kind = 0;
      const std::vector<int32_t> w = live ? written_segment(fp, t, static_cast<uint64_t>(b.keys[s]), &kind) : t;
      ++g_kinds[kind];
      if (static_cast<int64_t>(w.size()) != L) fail(name, "the written-out segment changes its length");
      for (int64_t j = 0; j < L; ++j) {
        want[at + j] = w[j];
        if (j + 1 < L) want_lab[at + j] = w[j + 1];
      }
    }
    for (int64_t i = 0; i < n; ++i) {
      if (out[i] != want[i]) {
        fail(name, "a token differs from the written-out layout");
        break;
      }
      if (lab[i] != want_lab[i]) {
        fail(name, "a label differs from the written-out layout");
        break;
      }
    }
  } else {
    // the soundness rule, written out position by position: a position belongs to a segment only if its id lies in
    // the capacity, its offset in the run and the whole run in its row; it then takes token pos of that run's
    // written-out layout, and every other position keeps its token and has no target
    for (int64_t i = 0; i < n; ++i) {
      const int64_t r = i / S, c = i % S, sg = b.seg[i], j = b.pos[i];
      int32_t want = b.ids[i];
      int64_t want_lab = -100;
      if (sg >= 0 && sg < b.cap && j >= 0 && j <= c) {
        const int64_t L = static_cast<int64_t>(b.cu[sg + 1]) - b.cu[sg], c0 = c - j;
        if (L >= 1 && j < L && c0 + L <= S) {
          const std::vector<int32_t> t(b.ids.begin() + r * S + c0, b.ids.begin() + r * S + c0 + L);
          int kind = 0;
          const std::vector<int32_t> w = live ? written_segment(fp, t, static_cast<uint64_t>(b.keys[sg]), &kind) : t;
          want = w[j];
          if (j + 1 < L) want_lab = w[j + 1];
        }
      }
      if (out[i] != want) {
        fail(name, "a token of a corrupt batch differs from the written-out soundness rule");
        break;
      }
      if (lab[i] != want_lab) {
        fail(name, "a label of a corrupt batch differs from the written-out soundness rule");
        break;
      }
    }
  }
  free(ids);
  free(cu);
  free(keys);
}

ddl::FimParams params(uint64_t ekey, double rate, double spm, bool has_eod, int32_t min_len) {
  return ddl::FimParams{ekey, static_cast<uint32_t>(rate * (1 << 24)), static_cast<uint32_t>(spm * (1 << 24)),
                        70001, 70002, 70003, 49999, has_eod ? 1 : 0, min_len};
}

}  // namespace

int main() {
  Lcg rng{2024};
  const int32_t eod = 49999;
  const std::vector<std::vector<int64_t>> len_sets = {
      {1, 3, 4, 5, 7, 8, 9, 26}, {4}, {5, 11}, {515, 516, 517, 1550, 3, 4}, {1 << 20}, {2, 6, 1029, 13, 510, 514}};
  for (int64_t S : {1, 3, 4, 8, 10, 511, 512, 516, 1024, 1030}) {
    for (const std::vector<int64_t>& lens : len_sets) {
      for (int64_t pad_tail : {int64_t{0}, int64_t{3}}) {
        const Batch b = make_batch(S > 600 ? 3 : 5, S, lens, pad_tail, eod, &rng);
        for (double rate : {0.0, 0.5, 1.0})
          for (double spm : {0.0, 0.5, 1.0})
            for (int has_eod = 0; has_eod < 2; ++has_eod)
              for (int32_t min_len : {4, 8})
                replay("grid", b, params(static_cast<uint64_t>(rng.next()) * 0x9E3779B97F4A7C15ull, rate, spm,
                                         has_eod != 0, min_len), true, true);
        replay("an invalid batch is copied", b, params(77, 1.0, 0.5, true, 4), false, true);
      }
    }
  }
  if (g_kinds[0] < 100 || g_kinds[1] < 100 || g_kinds[2] < 100) fail("grid", "a kind of segment is hardly covered");
  // corrupt batches: whatever the arrays hold, no index leaves its buffer and positions outside segments stay
  for (int c = 0; c < 300; ++c) {
    const int64_t S = 1 + rng.next() % 40;
    Batch b = make_batch(4, S, {3, 5, 9, 17}, 0, eod, &rng);
    for (int m = 0; m < 12; ++m) {
      const int64_t i = rng.next() % (b.R * b.S);
      switch (rng.next() % 5) {
        case 0: b.seg[i] = rng.next() % (2 * b.cap + 1) - b.cap / 2; break;
        case 1: b.pos[i] = rng.next() % (3 * S) - S; break;
        case 2: b.cu[rng.next() % b.cu.size()] = static_cast<int32_t>(rng.next() % (6 * S)) - static_cast<int32_t>(S); break;
        case 3: b.seg[i] = INT64_MAX - rng.next() % 2, b.pos[i] = INT64_MIN + rng.next() % 2; break;
        default: b.pos[i] = INT64_MAX - rng.next() % 3; break;
      }
    }
    if (c % 3 == 0 && b.cap > 1) {  // fewer keys than cu_seqlens entries: the capacity is the keys'
      b.keys.resize(b.cap / 2);
      b.cap = static_cast<int64_t>(b.keys.size());
      b.cu.resize(b.cap + 1);
    }
    replay("corrupt batch", b, params(static_cast<uint64_t>(rng.next()), 1.0, 0.5, c % 2 == 0, 4), true, false);
  }
  return finish("tokens fim check");
}
