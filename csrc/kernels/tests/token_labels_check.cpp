// Host check of the next-token label arithmetic of the indexed pad/pack kernel (ti_labels4 on top of ti_lane4,
// csrc/kernels/tokens_indexed.h), built with -fsanitize=address,undefined by tests/test_token_labels.py. It replays
// the kernel's lane loop with labels on (tokens_indexed.hip) for every lane of every workgroup, over hand-built and
// randomised plans: the corpus and the descriptor arrays are heap buffers of exactly their size, so the extra
// element a lane reads for its last position (the token at p0 + 4) is a heap overflow wherever it leaves the
// corpus. Every label source element must lie inside the selected sequence its position was read from, every
// label must be written exactly once, and the labels are compared with the definition applied by brute force to
// the batch a plain loop builds from the explicit flat stream. A corrupt descriptor (elements outside the corpus)
// must not be dereferenced, and its labels must still be the shifted ids the replay wrote.
#include <string.h>

#include "../tokens_indexed.h"
#include "check_common.h"

namespace {

int64_t g_fifth_loads = 0;  // label loads of the token at p0 + 4

Lcg g_rng{0x9E3779B97F4A7C15ull};
int64_t rnd(int64_t n) { return g_rng.next() % n; }  // [0, n)

// corrupt: 0 none; 1: every descriptor element moved so that the batch's reads straddle the corpus's end;
// 2: far outside (negative and beyond)
template <typename T>
void run_case(const char* name, const std::vector<int64_t>& lens, const std::vector<int64_t>& idx, int64_t S, int mode,
              int64_t fill_rows, int corrupt = 0) {
  ++g_cases;
  const int32_t pad_id = -7, ignore = -100;
  std::vector<int64_t> coffs(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) coffs[i + 1] = coffs[i] + lens[i];
  const int64_t corpus_elems = coffs.back();
  T* corpus = exact<T>(corpus_elems);
  std::vector<int64_t> seq_of(corpus_elems, -1);  // the corpus sequence of an element
  for (size_t i = 0; i < lens.size(); ++i)
    for (int64_t e = coffs[i]; e < coffs[i + 1]; ++e) seq_of[e] = static_cast<int64_t>(i);
  for (int64_t i = 0; i < corpus_elems; ++i) corpus[i] = static_cast<T>(i * 2654435761u + 12345u);
  std::vector<char> selected(lens.size(), 0);

  const int64_t n = static_cast<int64_t>(idx.size());
  std::vector<int64_t> offs_v(n + 1, 0), flat;
  int64_t* src_start = exact<int64_t>(n);
  for (int64_t i = 0; i < n; ++i) {
    src_start[i] = coffs[idx[i]];
    selected[idx[i]] = 1;
    offs_v[i + 1] = offs_v[i] + lens[idx[i]];
    for (int64_t p = 0; p < lens[idx[i]]; ++p) flat.push_back(static_cast<int64_t>(corpus[src_start[i] + p]));
  }
  std::vector<int64_t> rs_v, re_v, so_v;
  if (mode == 1) host_pack_plan(offs_v, S, &rs_v, &re_v, &so_v);
  const int64_t n_seg = mode == 1 ? static_cast<int64_t>(so_v.size()) - 1 : 0;
  const int64_t rows = mode == 1 ? static_cast<int64_t>(rs_v.size()) : n;
  int64_t* offsets = exact<int64_t>(n + 1);
  memcpy(offsets, offs_v.data(), (n + 1) * 8);
  int64_t* row_start = exact<int64_t>(rs_v.size());
  int64_t* row_end = exact<int64_t>(re_v.size());
  int64_t* seg_offsets = exact<int64_t>(so_v.size());
  int64_t* seg_src = exact<int64_t>(n_seg);
  if (!rs_v.empty()) memcpy(row_start, rs_v.data(), rs_v.size() * 8), memcpy(row_end, re_v.data(), re_v.size() * 8);
  if (!so_v.empty()) memcpy(seg_offsets, so_v.data(), so_v.size() * 8);
  for (int64_t s = 0, q = 0; s < n_seg; ++s) {  // the sequence that holds segment s (segments are never empty)
    while (!(offs_v[q] <= so_v[s] && so_v[s] < offs_v[q + 1])) ++q;
    seg_src[s] = src_start[q] + so_v[s] - offs_v[q];
  }
  if (corrupt) {
    for (int64_t i = 0; i < n; ++i)
      src_start[i] = corrupt == 1 ? corpus_elems - 1 - (i % 6) : (i % 2 ? -3 - i : corpus_elems + (int64_t{1} << 40) + i);
    for (int64_t s = 0; s < n_seg; ++s)
      seg_src[s] = corrupt == 1 ? corpus_elems - 1 - (s % 6) : (s % 2 ? -3 - s : corpus_elems + (int64_t{1} << 40) + s);
  }

  const int64_t R = fill_rows > rows ? fill_rows : rows;
  const int64_t total = R * S;
  int32_t* ids = exact<int32_t>(total);
  uint8_t* mask = exact<uint8_t>(total);
  int32_t* seg = exact<int32_t>(total);
  int64_t* labels = exact<int64_t>(total);
  std::vector<int> written(total, 0);

  // the kernel's load: an element outside the corpus is not dereferenced
  auto load = [&](int64_t e, int64_t same_as) -> int32_t {
    if (static_cast<uint64_t>(e) < static_cast<uint64_t>(corpus_elems)) {
      if (!corrupt) {
        if (!selected[seq_of[e]]) fail(name, "read outside the selected sequences");
        if (same_as >= 0 && seq_of[e] != seq_of[same_as]) fail(name, "label source outside its position's sequence");
      }
      return static_cast<int32_t>(corpus[e]);
    }
    if (!corrupt && e != -1) fail(name, "corpus index out of range");
    return pad_id;
  };

  // ---- the kernel with labels on, replayed
  const int64_t grid = ddl::ti_grid(rows, fill_rows, S, mode == 1);
  const int32_t chunks = static_cast<int32_t>(ddl::ti_chunks(S));
  if (grid < 0) fail(name, "grid overflow");
  std::vector<int64_t> seg_lds(ddl::kTiSegCap), src_lds(ddl::kTiSegCap);
  const bool staged = mode == 1 && n_seg + 1 <= ddl::kTiSegCap;
  if (staged)
    for (int64_t i = 0; i <= n_seg; ++i) {
      seg_lds[i] = seg_offsets[i];
      if (i < n_seg) src_lds[i] = seg_src[i];
    }
  for (int64_t bx = 0; bx < grid; ++bx)
    for (int tid = 0; tid < ddl::kTiThreads; ++tid) {
      int64_t row, p0;
      ddl::ti_lane_origin(static_cast<uint32_t>(bx), chunks, tid, &row, &p0);
      int64_t start = 0, len = 0, src0 = 0;
      if (row < rows) {
        if (mode == 0) {
          start = offsets[row];
          len = offsets[row + 1] - start;
          src0 = src_start[row];
        } else {
          start = row_start[row];
          len = row_end[row] - start;
        }
      }
      len = ddl::ti_row_len(len, S);
      if (row >= R || p0 >= S) continue;
      ddl::TiLane4 ln;
      ddl::TiLabel4 lb;
      if (staged) {
        const auto seg_at = [&](int64_t i) { return seg_lds[i]; };
        ddl::ti_lane4(mode, p0, start, len, src0, n_seg, seg_at, [&](int64_t i) { return src_lds[i]; }, &ln);
        ddl::ti_labels4(mode, p0, start, len, seg_at, ln, &lb);
      } else {
        const auto seg_at = [&](int64_t i) { return seg_offsets[i]; };  // exact size: entry n_seg + 1 overflows
        ddl::ti_lane4(mode, p0, start, len, src0, n_seg, seg_at, [&](int64_t i) { return seg_src[i]; }, &ln);
        ddl::ti_labels4(mode, p0, start, len, seg_at, ln, &lb);
      }
      int32_t tok[ddl::kTiLane], lab[ddl::kTiLane];
      for (int k = 0; k < ddl::kTiLane; ++k) tok[k] = load(ln.src[k], -1);
      for (int k = 0; k + 1 < ddl::kTiLane; ++k) {
        if (lb.has[k] && !corrupt && seq_of[ln.src[k + 1]] != seq_of[ln.src[k]])
          fail(name, "label source outside its position's sequence");
        lab[k] = lb.has[k] ? tok[k + 1] : ignore;
      }
      if (lb.has[3]) {
        ++g_fifth_loads;
        if (lb.src4 != ln.src[3] + 1) fail(name, "src4 is not the element after the lane's fourth");
        lab[3] = load(lb.src4, ln.src[3]);
      } else {
        if (lb.src4 != -1) fail(name, "src4 set without a label");
        lab[3] = ignore;
      }
      const int64_t o = row * S + p0;
      const int cnt = ddl::ti_vector_store(p0, S) ? ddl::kTiLane : static_cast<int>(S - p0 < 4 ? S - p0 : 4);
      if (ddl::ti_vector_store(p0, S) && o % 2) fail(name, "unaligned 16-byte label store");
      for (int k = 0; k < cnt; ++k) {
        ids[o + k] = tok[k];
        mask[o + k] = ln.msk[k];
        seg[o + k] = ln.seg[k];
        labels[o + k] = lab[k];
        ++written[o + k];
      }
    }

  // ---- the definition, by brute force
  bool ok = true;
  for (int64_t r = 0; r < R; ++r) {
    int64_t start = 0, len = 0;
    if (r < rows) {
      start = mode == 0 ? offs_v[r] : rs_v[r];
      len = (mode == 0 ? offs_v[r + 1] : re_v[r]) - start;
      if (len > S) len = S;
    }
    std::vector<int32_t> e_tok(S, pad_id), e_seg(S, mode == 0 ? 0 : -1);
    std::vector<uint8_t> e_msk(S, 0);
    for (int64_t p = 0; p < S; ++p) {
      if (corrupt) {  // the other outputs are whatever the replay wrote: the labels are a function of them
        e_tok[p] = ids[r * S + p], e_seg[p] = seg[r * S + p], e_msk[p] = mask[r * S + p];
      } else if (p < len) {
        const int64_t g = start + p;
        e_tok[p] = static_cast<int32_t>(flat[g]);
        e_msk[p] = 1;
        if (mode == 1) {
          int64_t s = 0;
          while (so_v[s + 1] <= g) ++s;
          e_seg[p] = static_cast<int32_t>(s);
        }
      }
    }
    for (int64_t p = 0; p < S; ++p) {
      int64_t e_lab = ignore;
      if (p + 1 < S && e_msk[p + 1] == 1 && (mode == 0 || e_seg[p + 1] == e_seg[p])) e_lab = e_tok[p + 1];
      const int64_t o = r * S + p;
      ok = ok && written[o] == 1 && labels[o] == e_lab && ids[o] == e_tok[p] && mask[o] == e_msk[p] &&
           seg[o] == e_seg[p];
    }
  }
  if (!ok) {
    printf("%s (elem %d B, S %lld, mode %d, fill %lld, corrupt %d): mismatch\n", name, static_cast<int>(sizeof(T)),
           (long long)S, mode, (long long)fill_rows, corrupt);
    ++g_failures;
  }
  for (void* p : {(void*)corpus, (void*)src_start, (void*)offsets, (void*)row_start, (void*)row_end,
                  (void*)seg_offsets, (void*)seg_src, (void*)ids, (void*)mask, (void*)seg, (void*)labels})
    free(p);
}

template <typename T>
void run_all() {
  // segment ends at positions = 3 and = 0 mod 4 of a row, one-token and empty sequences; the corpus's last
  // sequence, which ends at the corpus's last element, is selected last and first
  const std::vector<int64_t> lens = {4, 1, 0, 5, 8, 3, 1, 1, 0, 12, 2, 9};
  std::vector<int64_t> all, rev;
  for (size_t i = 0; i < lens.size(); ++i) all.push_back(static_cast<int64_t>(i)), rev.push_back(lens.size() - 1 - i);
  for (int64_t S : {4, 5, 8, 16, 37})
    for (int mode : {0, 1}) {
      run_case<T>("boundaries", lens, all, S, mode, 0);
      run_case<T>("boundaries, reversed", lens, rev, S, mode, 0);
      run_case<T>("boundaries, padding rows", lens, all, S, mode, mode == 1 ? 20 : 0);
    }
  // a segment whose last token is at position 511 of a row (the next one starts the second chunk), and at 512
  for (int64_t S : {520, 515, 1024})
    for (int mode : {0, 1}) {
      run_case<T>("end at 511", {512, 3, 512, 600}, {0, 1, 2, 3}, S, mode, 0);
      run_case<T>("end at 512", {513, 2, 513, 513}, {0, 1, 2, 3}, S, mode, 0);
      run_case<T>("end at 511, last of the corpus", {7, 512}, {1}, S, mode, 0);
      run_case<T>("end at 512, last of the corpus", {7, 513}, {0, 1}, S, mode, 0);
    }
  // n_seg + 1 on both sides of kTiSegCap: 1022 / 1023 segments are searched in LDS, 1024 / 1100 in global memory
  for (int64_t n : {1022, 1023, 1024, 1100}) {
    std::vector<int64_t> small, small_idx;
    for (int64_t i = 0; i < n; ++i) small.push_back(1 + i % 3), small_idx.push_back((i * 7) % n);
    run_case<T>("around the LDS cap", small, small_idx, 16, 1, 0);
    run_case<T>("around the LDS cap, pad", small, small_idx, 16, 0, 0);
  }
  for (int mode : {0, 1}) {
    run_case<T>("all empty", {0, 0, 3}, {0, 1, 0}, 16, mode, 0);
    run_case<T>("n = 0", {4, 5}, {}, 16, mode, 0);
  }
  run_case<T>("n = 0, padding rows", {4, 5}, {}, 516, 1, 2);
  // corrupt descriptors: straddling the corpus's end, and far outside on both sides
  for (int corrupt : {1, 2})
    for (int mode : {0, 1})
      for (int64_t S : {8, 37, 520}) run_case<T>("corrupt", {600, 9, 0, 5, 17, 1030}, {5, 1, 2, 3, 4, 0}, S, mode, 0, corrupt);
  // randomised plans: lengths in [0, 3 S], repeats, padding rows
  for (int it = 0; it < 60; ++it) {
    const int64_t S = it % 5 == 4 ? 500 + rnd(40) : 3 + rnd(45);
    const int64_t nc = 1 + rnd(it % 5 == 4 ? 12 : 70);
    std::vector<int64_t> rl, ri;
    for (int64_t i = 0; i < nc; ++i) rl.push_back(rnd(4) == 0 ? rnd(3) : rnd(3 * S + 1));
    rl.push_back(1 + rnd(2 * S));  // the corpus's last sequence: non-empty, and selected
    const int64_t n = rnd(nc + 8);
    for (int64_t i = 0; i < n; ++i) ri.push_back(rnd(nc + 1));
    ri.push_back(nc);
    const int mode = static_cast<int>(rnd(2));
    run_case<T>("random", rl, ri, S, mode, mode == 1 && rnd(2) ? rnd(2 * n + 4) : 0);
  }
}

}  // namespace

int main() {
  run_all<uint16_t>();
  run_all<int32_t>();
  if (g_fifth_loads == 0) fail("token labels check", "no lane ever loaded the token at p0 + 4");
  char note[64];
  snprintf(note, sizeof note, " (%lld fifth-token loads)", (long long)g_fifth_loads);
  return finish("token labels check", note);
}
