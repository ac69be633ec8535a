// Host check of the indexed pad/pack kernel's index arithmetic (csrc/kernels/tokens_indexed.h), built with
// -fsanitize=address,undefined by tests/test_resident_tokens.py. It replays the kernel's loops
// (tokens_indexed.hip) workgroup by workgroup, lane by lane, on the host: the corpus, the descriptor arrays and
// every output are heap buffers of exactly their size, so an element read outside the corpus, a descriptor
// entry past its array or a store outside an output [R, S] is a heap overflow. A read inside the corpus but
// outside the selected sequences is counted as a failure, every output element must be written exactly once,
// and the result is compared with a plain loop over the explicitly built flat stream.
#include <string.h>

#include "../tokens_indexed.h"
#include "check_common.h"

namespace {

template <typename T, typename P>
void run_case(const char* name, const std::vector<int64_t>& lens, const std::vector<int64_t>& idx, int64_t S, int mode,
              int64_t fill_rows) {
  ++g_cases;
  const int32_t pad_id = -7;
  std::vector<int64_t> coffs(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) coffs[i + 1] = coffs[i] + lens[i];
  const int64_t corpus_elems = coffs.back();
  T* corpus = exact<T>(corpus_elems);
  for (int64_t i = 0; i < corpus_elems; ++i) corpus[i] = static_cast<T>(i * 2654435761u + 12345u);
  std::vector<char> may_read(corpus_elems, 0);

  const int64_t n = static_cast<int64_t>(idx.size());
  std::vector<int64_t> offs_v(n + 1, 0), flat;
  int64_t* src_start = exact<int64_t>(n);
  for (int64_t i = 0; i < n; ++i) {
    src_start[i] = coffs[idx[i]];
    offs_v[i + 1] = offs_v[i] + lens[idx[i]];
    for (int64_t p = 0; p < lens[idx[i]]; ++p) {
      may_read[src_start[i] + p] = 1;
      flat.push_back(static_cast<int64_t>(corpus[src_start[i] + p]));  // widened: T is unsigned 16-bit or int32
    }
  }
  std::vector<int64_t> rs_v, re_v, so_v;
  if (mode == 1) host_pack_plan(offs_v, S, &rs_v, &re_v, &so_v);
  const int64_t n_seg = mode == 1 ? static_cast<int64_t>(so_v.size()) - 1 : 0;
  const int64_t rows = mode == 1 ? static_cast<int64_t>(rs_v.size()) : n;
  // exact-size descriptor arrays, as the op uploads them
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

  const int64_t R = fill_rows > rows ? fill_rows : rows;
  const int64_t total = R * S;
  int32_t* ids = exact<int32_t>(total);
  uint8_t* mask = exact<uint8_t>(total);
  P* pos = exact<P>(total);
  int32_t* seg = exact<int32_t>(total);
  int32_t* cu = exact<int32_t>(mode == 1 ? n_seg + 1 : 0);
  std::vector<int> written(total, 0), cu_written(mode == 1 ? n_seg + 1 : 0, 0);

  // ---- the kernel, replayed
  const bool has_cu = mode == 1;
  const int64_t grid = ddl::ti_grid(rows, fill_rows, S, has_cu);
  const int32_t chunks = static_cast<int32_t>(ddl::ti_chunks(S));
  if (grid < 0) fail(name, "grid overflow");
  std::vector<int64_t> seg_lds(ddl::kTiSegCap), src_lds(ddl::kTiSegCap);
  for (int64_t bx = 0; bx < grid; ++bx) {
    const bool staged = mode == 1 && n_seg + 1 <= ddl::kTiSegCap;
    for (int tid = 0; tid < ddl::kTiThreads; ++tid) {  // the staging loops, before the barrier
      int64_t row, p0;
      ddl::ti_lane_origin(static_cast<uint32_t>(bx), chunks, tid, &row, &p0);
      const bool live = row < R;
      if (staged && live)
        for (int64_t i = tid; i <= n_seg; i += ddl::kTiThreads) {
          seg_lds[i] = seg_offsets[i];
          if (i < n_seg) src_lds[i] = seg_src[i];
        }
      if (has_cu && bx == 0)
        for (int64_t i = tid; i <= n_seg; i += ddl::kTiThreads) {
          cu[i] = static_cast<int32_t>(seg_offsets[i]);
          ++cu_written[i];
        }
    }
    for (int tid = 0; tid < ddl::kTiThreads; ++tid) {
      int64_t row, p0;
      ddl::ti_lane_origin(static_cast<uint32_t>(bx), chunks, tid, &row, &p0);
      const bool live = row < R;
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
      if (!live || p0 >= S) continue;
      ddl::TiLane4 ln;
      if (staged)
        ddl::ti_lane4(mode, p0, start, len, src0, n_seg, [&](int64_t i) { return seg_lds[i]; },
                      [&](int64_t i) { return src_lds[i]; }, &ln);
      else
        ddl::ti_lane4(mode, p0, start, len, src0, n_seg, [&](int64_t i) { return seg_offsets[i]; },
                      [&](int64_t i) { return seg_src[i]; }, &ln);
      int32_t tok[ddl::kTiLane];
      for (int k = 0; k < ddl::kTiLane; ++k) {
        const int64_t e = ln.src[k];
        if (static_cast<uint64_t>(e) < static_cast<uint64_t>(corpus_elems)) {
          if (!may_read[e]) fail(name, "read outside the selected sequences");
          tok[k] = static_cast<int32_t>(corpus[e]);
        } else {
          if (e != -1) fail(name, "corpus index out of range");
          tok[k] = pad_id;
        }
      }
      const int64_t o = row * S + p0;
      const int cnt = ddl::ti_vector_store(p0, S) ? ddl::kTiLane : static_cast<int>(S - p0 < 4 ? S - p0 : 4);
      if (ddl::ti_vector_store(p0, S) && o % 4) fail(name, "unaligned vector store");
      for (int k = 0; k < cnt; ++k) {
        ids[o + k] = tok[k];
        mask[o + k] = ln.msk[k];
        pos[o + k] = static_cast<P>(ln.pos[k]);
        seg[o + k] = ln.seg[k];
        ++written[o + k];
      }
    }
  }

  // ---- the plain loop over the flat stream
  bool ok = true;
  for (int64_t r = 0; r < R && ok; ++r) {
    int64_t start = 0, len = 0;
    if (r < rows) {
      start = mode == 0 ? offs_v[r] : rs_v[r];
      len = (mode == 0 ? offs_v[r + 1] : re_v[r]) - start;
      if (len > S) len = S;
    }
    for (int64_t p = 0; p < S; ++p) {
      int32_t e_tok = pad_id, e_seg = mode == 0 ? 0 : -1;
      int64_t e_pos = 0;
      const uint8_t e_msk = p < len;
      if (p < len) {
        const int64_t g = start + p;
        e_tok = static_cast<int32_t>(flat[g]);
        if (mode == 0) {
          e_pos = p;
        } else {
          int64_t s = 0;
          while (so_v[s + 1] <= g) ++s;
          e_pos = g - so_v[s];
          e_seg = static_cast<int32_t>(s);
        }
      }
      const int64_t o = r * S + p;
      ok = ok && written[o] == 1 && ids[o] == e_tok && mask[o] == e_msk && static_cast<int64_t>(pos[o]) == e_pos &&
           seg[o] == e_seg;
    }
  }
  for (int64_t i = 0; mode == 1 && i <= n_seg; ++i) ok = ok && cu_written[i] == 1 && cu[i] == so_v[i];
  if (!ok) {
    printf("%s (elem %d B, S %lld, mode %d, fill %lld): mismatch\n", name, static_cast<int>(sizeof(T)), (long long)S,
           mode, (long long)fill_rows);
    ++g_failures;
  }
  for (void* p : {(void*)corpus, (void*)src_start, (void*)offsets, (void*)row_start, (void*)row_end,
                  (void*)seg_offsets, (void*)seg_src, (void*)ids, (void*)mask, (void*)pos, (void*)seg, (void*)cu})
    free(p);
}

template <typename T>
void run_all() {
  // the ragged corpus of the GPU test: the wanted lengths, each behind a filler that walks the start residues
  // modulo 8 elements; the corpus's first and last sequence and two repeated indices
  const std::vector<int64_t> wanted = {0, 1, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1000, 0, 5};
  std::vector<int64_t> lens, idx;
  lens.push_back(6);
  int64_t at = 6;
  for (size_t i = 0; i < wanted.size(); ++i) {
    const int64_t fill = ((static_cast<int64_t>(i) - at) % 8 + 8) % 8;
    lens.push_back(fill);
    lens.push_back(wanted[i]);
    at += fill + wanted[i];
    idx.push_back(static_cast<int64_t>(lens.size()) - 1);
  }
  lens.push_back(11);
  idx.push_back(0);
  idx.push_back(static_cast<int64_t>(lens.size()) - 1);
  idx.push_back(idx[9]);
  idx.push_back(idx[12]);
  for (int64_t S : {6, 256, 512, 516})
    for (int mode : {0, 1}) {
      run_case<T, int64_t>("ragged", lens, idx, S, mode, 0);
      run_case<T, int32_t>("ragged i32 positions", lens, idx, S, mode, 0);
    }
  run_case<T, int64_t>("ragged, padding rows", lens, idx, 256, 1, 40);
  run_case<T, int64_t>("ragged, fewer fill rows than rows", lens, idx, 6, 1, 3);
  // plans around the LDS cap of the segment search
  std::vector<int64_t> many = mod_lens(1100, 13), many_idx = stride_order(1100, 7, 0, 1100);
  run_case<T, int64_t>("many", many, many_idx, 37, 1, 0);  // 1015 segments: just under the cap
  run_case<T, int64_t>("many, pad", many, many_idx, 37, 0, 0);
  run_case<T, int64_t>("many, short rows", many, many_idx, 6, 1, 0);  // ~1520 segments: searched in global memory
  for (int64_t i = 1100; i < 1200; ++i) {
    many.push_back(i % 13);
    many_idx.push_back(i);
  }
  run_case<T, int64_t>("more", many, many_idx, 37, 1, 0);  // 1107 segments
  std::vector<int64_t> ones(1023, 1), ones_idx;  // kTiSegCap - 1 segments: the largest plan that is staged
  for (int64_t i = 0; i < 1023; ++i) ones_idx.push_back(1022 - i);
  run_case<T, int64_t>("cap - 1 segments", ones, ones_idx, 37, 1, 0);
  ones.push_back(1);
  ones_idx.push_back(1023);
  run_case<T, int64_t>("cap segments", ones, ones_idx, 37, 1, 0);
  for (int mode : {0, 1}) {
    run_case<T, int64_t>("all empty", {0, 0, 3}, {0, 1, 0}, 16, mode, 0);
    run_case<T, int64_t>("n = 0", {4, 5}, {}, 16, mode, 0);
  }
  run_case<T, int64_t>("all empty, padding rows", {0, 0, 3}, {0, 1, 0}, 16, 1, 5);
  run_case<T, int64_t>("n = 0, padding rows", {4, 5}, {}, 516, 1, 2);
}

}  // namespace

int main() {
  run_all<uint16_t>();
  run_all<int32_t>();
  return finish("tokens indexed check");
}
