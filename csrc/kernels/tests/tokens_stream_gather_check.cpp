// Host check of the stream piece gather (csrc/kernels/tokens_stream_gather.h), built with -fsanitize=address,undefined
// by tests/test_stream_gather_check.py. It replays the kernel's loops (tokens_stream_gather.hip) chunk by chunk, group
// by group, lane by lane on the host with the shared header; only the wave collectives have a stand-in (the wave-wide
// search: replay_search; the scan of the unit counts: a serial sum). The plan arrays are read through views that check
// every index, every 16-byte unit load is a memcpy out of a source buffer that is exactly the 16-byte aligned hull of
// the corpus, and every store goes into a window of exactly rows * S elements. The check asserts that every position
// below min(seg_offsets[n_seg], rows * S) whose piece lies inside the corpus is written exactly once with the right
// element and nothing else is written, and that the units read are exactly the hulls of the clipped pieces, computed
// here by plain arithmetic over all (piece, chunk) pairs. The far cases run the same replay with no memory behind the
// addresses and check every unit and element address instead.
#include <string.h>

#include <map>

#include "../tokens_stream_gather.h"
#include "stream_check_common.h"

namespace {

struct Plan {
  std::vector<int64_t> seg_src, seg_offsets;  // n_seg and n_seg + 1 entries
  int64_t n_rows;                             // counts[0]
  int64_t n_seg() const { return static_cast<int64_t>(seg_src.size()); }
};

// documents (first corpus element, length) back to back, cut at every multiple of S: the pieces of a stream plan
Plan make_plan(const std::vector<int64_t>& doc_src, const std::vector<int64_t>& doc_len, int64_t S) {
  Plan p;
  int64_t g = 0;
  for (size_t i = 0; i < doc_src.size(); ++i) {
    int64_t done = 0;
    while (done < doc_len[i]) {
      const int64_t room = S - g % S, left = doc_len[i] - done;
      const int64_t n = left < room ? left : room;
      p.seg_offsets.push_back(g);
      p.seg_src.push_back(doc_src[i] + done);
      g += n;
      done += n;
    }
  }
  p.seg_offsets.push_back(g);
  p.n_rows = (g + S - 1) / S;
  return p;
}

// `far`: src is a synthetic address with no memory behind it
template <typename T>
void replay(const char* name, const Plan& plan, int64_t corpus_elems, int shift, uint64_t far_src, int64_t max_segs,
            int64_t rows, int64_t S, int64_t max_blocks) {
  ++g_cases;
  constexpr int eb = static_cast<int>(sizeof(T));
  constexpr int per_unit = ddl::kRgUnitBytes / eb;
  const bool far = far_src != 0;
  // the corpus starts `shift` elements into a 16-byte aligned allocation that is exactly its hull
  const size_t hull_bytes = far ? 16 : (static_cast<size_t>(shift + corpus_elems) * eb + 15) / 16 * 16;
  uint8_t* raw = static_cast<uint8_t*>(aligned_alloc(16, hull_bytes ? hull_bytes : 16));
  for (size_t i = 0; i < hull_bytes; ++i) raw[i] = static_cast<uint8_t>(i * 131u + 7u);
  const uint64_t src = far ? far_src : reinterpret_cast<uint64_t>(raw) + static_cast<uint64_t>(shift) * eb;

  // the plan in buffers of the capacity's size, as the plan kernels leave it: entries past n_seg are never written
  const int64_t n_seg = plan.n_seg();
  const int64_t held = n_seg <= max_segs ? n_seg : 0;  // an overflowed plan holds nothing the kernel may read
  int64_t* seg_src = exact<int64_t>(held);
  int64_t* seg_offsets = exact<int64_t>(held + 1);
  for (int64_t i = 0; i < held; ++i) seg_src[i] = plan.seg_src[i];
  for (int64_t i = 0; i <= held; ++i) seg_offsets[i] = held ? plan.seg_offsets[i] : 0;
  const View so{seg_offsets, held + 1, name, "seg_offsets read out of range"};
  const View ss{seg_src, held, name, "seg_src read out of range"};
  const int64_t counts[2] = {plan.n_rows, n_seg};

  const int64_t win = rows * S;
  T* dst = exact<T>(far ? 0 : win);
  std::vector<int> written(win, 0);
  std::map<uint64_t, int> loads;

  // the kernel ---------------------------------------------------------------------------------------------------
  const int64_t grid_chunks = ddl::sg_chunks(win, eb);
  const int64_t grid = (max_blocks > 0 && max_blocks < grid_chunks) ? max_blocks : grid_chunks;
  for (int64_t block = 0; block < grid; ++block) {
    if (!ddl::sg_plan_ok(counts[0], counts[1], max_segs)) continue;
    const int64_t limit = ddl::sg_limit(counts[0], rows, S, so[n_seg]);
    const int64_t n_chunks = ddl::sg_chunks(limit, eb);
    for (int64_t c = block; c < n_chunks; c += grid) {
      int64_t c0, c1;
      ddl::sg_chunk(c, limit, eb, &c0, &c1);
      if (c1 <= c0) fail(name, "an empty chunk");
      const int64_t s0 = replay_search(name, seg_offsets, n_seg, c0);
      const int64_t s1 = replay_search(name, seg_offsets, n_seg, c1 - 1);
      for (int64_t gb = s0; gb <= s1; gb += ddl::kSgGroup) {
        ddl::SgPiece p[ddl::kSgGroup];
        int64_t upre[ddl::kSgGroup + 1];
        upre[0] = 0;
        for (int tid = 0; tid < ddl::kSgGroup; ++tid) {
          p[tid] = ddl::SgPiece{0, 0, 0, 0};
          if (gb + tid <= s1) p[tid] = ddl::sg_piece(so, ss, gb + tid, n_seg, c0, c1, src, corpus_elems, eb);
          upre[tid + 1] = upre[tid] + p[tid].units;  // the scan's stand-in
        }
        const int64_t total = upre[ddl::kSgGroup];
        const auto upre_at = [&](int64_t j) {
          if (j < 0 || j > ddl::kSgGroup) fail(name, "unit prefix read out of range");
          return upre[j];
        };
        for (int64_t base = 0; base < total; base += ddl::kRgTileUnits) {
          for (int tid = 0; tid < ddl::kRgThreads; ++tid) {
            T v[ddl::kRgUnroll][per_unit];
            int64_t pj[ddl::kRgUnroll], pu[ddl::kRgUnroll];
            for (int k = 0; k < ddl::kRgUnroll; ++k) {
              const int64_t w = ddl::sg_unit(base, k, tid);
              pj[k] = -1;
              if (w >= total) continue;
              const int64_t j = pj[k] = ddl::sg_unit_piece(upre_at, ddl::kSgGroup, w);
              if (j < 0 || j >= ddl::kSgGroup || w < upre[j] || w >= upre[j + 1]) {
                fail(name, "unit mapped to a wrong piece");
                pj[k] = -1;
                continue;
              }
              pu[k] = w - upre[j];
              const uint64_t ua = ddl::rg_unit_addr(p[j].a, pu[k]);
              if (ua % 16) fail(name, "unaligned unit");
              ++loads[ua];
              if (!far) memcpy(v[k], reinterpret_cast<const void*>(ua), 16);  // the whole unit, as the lane's load
            }
            for (int k = 0; k < ddl::kRgUnroll; ++k) {
              if (pj[k] < 0) continue;
              const ddl::SgPiece& q = p[pj[k]];
              const int64_t head = ddl::rg_head_elems(q.a, eb);
              for (int e = 0; e < per_unit; ++e) {
                const int64_t pos = ddl::rg_elem_pos(pu[k], e, head, eb);
                if (pos < 0 || pos >= q.len) continue;
                const int64_t g = q.d0 + pos;
                if (g < 0 || g >= win) {
                  fail(name, "store outside the window");
                  continue;
                }
                if (far) {
                  const uint64_t want = src + static_cast<uint64_t>(plan.seg_src[gb + pj[k]] +
                                                                    (g - plan.seg_offsets[gb + pj[k]])) * eb;
                  if (ddl::rg_unit_addr(q.a, pu[k]) + static_cast<uint64_t>(e) * eb != want)
                    fail(name, "element address");
                } else {
                  dst[g] = v[k][e];
                }
                ++written[g];
              }
            }
          }
        }
      }
    }
  }

  // what it must have done, by plain arithmetic ----------------------------------------------------------------------
  const bool ok_plan = plan.n_rows > 0 && n_seg > 0 && n_seg <= max_segs;
  int64_t limit = 0;
  if (ok_plan) {
    limit = plan.seg_offsets[n_seg];
    const int64_t cap = (plan.n_rows < rows ? plan.n_rows : rows) * S;
    if (cap < limit) limit = cap;
  }
  std::map<uint64_t, int> want_loads;
  std::vector<int> want_written(win, 0);
  const int64_t ce = ddl::kSgChunkBytes / eb;
  for (int64_t s = 0; ok_plan && s < n_seg; ++s) {
    const int64_t lo = plan.seg_offsets[s], hi = plan.seg_offsets[s + 1], e0 = plan.seg_src[s];
    if (e0 < 0 || e0 + (hi - lo) > corpus_elems) continue;  // outside the corpus: not dereferenced, not written
    for (int64_t c0 = lo / ce * ce; c0 < hi && c0 < limit; c0 += ce) {
      const int64_t c1 = c0 + ce < limit ? c0 + ce : limit;
      const int64_t g0 = lo > c0 ? lo : c0, g1 = hi < c1 ? hi : c1;
      if (g1 <= g0) continue;
      const uint64_t b0 = src + static_cast<uint64_t>(e0 + (g0 - lo)) * eb, b1 = b0 + static_cast<uint64_t>(g1 - g0) * eb;
      for (uint64_t ua = b0 & ~uint64_t{15}; ua < b1; ua += 16) ++want_loads[ua];
      for (int64_t g = g0; g < g1; ++g) {
        ++want_written[g];
        if (!far && memcmp(&dst[g], reinterpret_cast<const void*>(src + static_cast<uint64_t>(e0 + (g - lo)) * eb), eb))
          fail(name, "wrong element");
      }
    }
  }
  if (written != want_written) fail(name, "a position is not written exactly once (or one that must stay is written)");
  if (loads != want_loads) fail(name, "the units read are not the hulls of the clipped pieces");
  if (g_failures) printf("  (%s: eb %d, shift %d, max_blocks %lld)\n", name, eb, shift, (long long)max_blocks);
  free(dst);
  free(seg_src);
  free(seg_offsets);
  free(raw);
}

// documents of the given lengths back to back in a corpus that starts with `lead` other elements and ends with the
// last document
template <typename T>
void docs_case(const char* name, const std::vector<int64_t>& lens, int64_t lead, int shift, int64_t S, int64_t rows,
               int64_t max_blocks, int64_t max_segs = 1 << 30) {
  std::vector<int64_t> src;
  int64_t at = lead;
  for (int64_t n : lens) {
    src.push_back(at);
    at += n;
  }
  replay<T>(name, make_plan(src, lens, S), at, shift, 0, max_segs, rows, S, max_blocks);
}

template <typename T>
void run_all() {
  constexpr int eb = static_cast<int>(sizeof(T));
  constexpr int per_unit = 16 / eb;
  const int64_t ce = ddl::sg_chunk_elems(eb);
  // every alignment of a piece's first element inside a 16-byte unit, for short lengths around a unit
  for (int shift = 0; shift < per_unit; ++shift)
    for (int64_t len : {int64_t{1}, int64_t{2}, int64_t{per_unit - 1}, int64_t{per_unit}, int64_t{per_unit + 1},
                        int64_t{3 * per_unit + 1}})
      for (int64_t lead : {0, 1, 3}) docs_case<T>("alignments", {len, 5, len}, lead, shift, 64, 4, 0);
  // pieces of 1 element, more of them in one chunk than a workgroup has lanes; S = 4 cuts nothing further
  docs_case<T>("1-element pieces", std::vector<int64_t>(700, 1), 0, 1, 4, 175, 0);
  docs_case<T>("1-element pieces, two chunks", std::vector<int64_t>(static_cast<size_t>(ce + 300), 1), 3, 0, 60,
               (ce + 300 + 59) / 60, 1);
  // the odd row widths of the GPU test: documents of 0 (none), 1, S, 3 S + 1 tokens
  for (int64_t S : {4, 60, 64})
    for (int64_t rows : {1, 3}) docs_case<T>("row widths", {1, S, 3 * S + 1, 1, S, 2}, 2, 3, S, rows, 0);
  // a piece that ends exactly on a unit and on a chunk boundary (aligned source), and its unaligned twin
  docs_case<T>("ends on a chunk boundary", {ce, 40}, 0, 0, 2 * ce, 2, 0);
  docs_case<T>("ends on a chunk boundary, unaligned", {ce, 40}, 5, 1, 2 * ce, 2, 0);
  // a piece spanning three chunks, its ends inside units; grid-stride with one and with two workgroups
  for (int64_t mb : {0, 1, 2}) docs_case<T>("three chunks", {ce - 50, 2 * ce + 100, 77}, 7, 1, 4 * ce, 1, mb);
  // a window reaching past the stream's end, and one shorter than the plan's tokens (the capacity clamps)
  docs_case<T>("past the end", {100, 30}, 0, 0, 64, 8, 0);
  docs_case<T>("capacity below the plan", {100, 300, 100}, 0, 2, 64, 3, 0);
  // nothing to do: no piece, a negative row count, a plan beyond its capacity (whose arrays hold nothing)
  docs_case<T>("n_seg = 0", {}, 10, 0, 64, 2, 0);
  {
    Plan p = make_plan({0, 50}, {50, 70}, 64);
    p.n_rows = -1;
    replay<T>("negative rows", p, 120, 0, 0, 1 << 30, 2, 64, 0);
  }
  docs_case<T>("overflowed plan", {50, 70, 9}, 0, 0, 64, 3, 0, 2);
  // pieces whose source lies outside the corpus are skipped, their neighbours copied
  {
    Plan p = make_plan({0, -3, 40, 190, 100, 1000}, {20, 20, 20, 20, 20, 20}, 64);
    replay<T>("seg_src outside the corpus", p, 200, 1, 0, 1 << 30, 2, 64, 0);
  }
  // the first piece at corpus element 0 and the last ending at corpus_elems: the hulls stay inside the corpus's own
  docs_case<T>("corpus edges", {3, 2 * ce + 1}, 0, 0, 64, (2 * ce + 4 + 63) / 64, 0);
  // far: synthetic base addresses past 2^32 and 2^40 bytes, pieces whose byte offsets pass 2^33 and 2^41
  for (uint64_t base : {(uint64_t{1} << 32) + 48, (uint64_t{0x7f} << 40)})
    for (int shift : {0, 1, 3}) {
      const int64_t far = (int64_t{1} << 33) / eb;
      Plan p = make_plan({far - 3, (int64_t{1} << 41) / eb + 1, 5, 2 * far + 7}, {5000, ce + 17, 1, 9000}, 4096);
      replay<T>("far", p, (int64_t{1} << 42), shift, base + static_cast<uint64_t>(shift) * eb, 1 << 30, 8, 4096, 3);
    }
}

}  // namespace

int main() {
  run_all<uint16_t>();
  run_all<uint32_t>();
  return finish("stream gather check");
}
